"""Rows slabs for the rows forms of the slab fills, seeds that satisfy only their contract, and the plain statements of what each rows
form makes of them (no GPU, no use of the library).  The sibling of tests/slab_value_cases.py, whose generators make the values.

A rows slab is what the rows walk fills: ``f64[m][n]``, row k the values of the call's query genome ``rows[k]`` to every genome.
``hip.set_rows_values`` (the test-hooks twin) puts any such array in its place, EVERY element of it.  Which elements a rows form may read:

* the flat passes (edges, components, tree) read the LIVE elements: ``[k][g]`` with ``g > rows[k]``, or ``g < rows[k]`` and g no query
  genome.  The diagonal ``[k][rows[k]]`` is no pair, and of the two copies of a pair of two query genomes the one in the row of the
  larger is never read (the DEAD copy);
* the nearest fill reads every element but the diagonal: a query genome's list is made of its own row, so both copies count, each in
  its own row's list.

``poisoned`` puts into the diagonal and the dead copies a value that would change the result if it were read.  Every reference takes
``read="live"`` (the statement) or ``read="all"`` (what a kernel that read the poison would make of it): tests/test_rows_values_host.py
shows that the two differ on the inputs tests/rows_values_driver.py runs, so a kernel that read a dead element could not pass.

The references are numpy and pure Python over int64 millionths and f64 bit patterns.  tests/test_rows_values_host.py holds each to the
host statements the project already trusts (``SparseEdges`` / ``Components`` / ``SingleLinkageTree`` / ``NearestNeighbors``
``.extended`` and ``.from_dense``)."""

import numpy as np

import slab_value_cases as tri

MILLION = tri.MILLION
CHUNK = 4096                           # elements one workgroup of a flat pass covers (SLAB_CHUNK)


class Refused(Exception):
    """A value the tree fill must refuse (no millionth in [0, 1]) among the elements read; ``args[0]``: how many."""


# ---- the slab --------------------------------------------------------------------------------------------------------
def as_rows(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    assert (np.diff(rows) > 0).all(), "rows ascend strictly"
    return rows


def query_mask(rows, n):
    mask = np.zeros(n, dtype=bool)
    mask[as_rows(rows)] = True
    return mask


def rows_of(triangle, n, rows):
    """The symmetric rows slab of a value triangle: row k is row rows[k] of the square (the diagonal holds 0.0)."""
    return np.ascontiguousarray(tri.square(np.asarray(triangle, dtype=np.float64), n, diagonal=0.0)[as_rows(rows)])


def diagonal_mask(rows, n):
    rows = as_rows(rows)
    mask = np.zeros((rows.shape[0], n), dtype=bool)
    mask[np.arange(rows.shape[0]), rows] = True
    return mask


def dead_mask(rows, n):
    """[k][g] with g < rows[k] and g a query genome: the copy of a pair of two query genomes that the flat passes must not read."""
    rows = as_rows(rows)
    g = np.arange(n, dtype=np.int64)[None, :]
    return (g < rows[:, None]) & query_mask(rows, n)[None, :]


def live_mask(rows, n):
    """The elements the flat passes read: everything but the diagonal and the dead copies."""
    return ~(diagonal_mask(rows, n) | dead_mask(rows, n))


def poisoned(slab, rows, n, diagonal, dead=None):
    """A copy of the slab with ``diagonal`` in every diagonal element and, when given, ``dead`` in every dead copy."""
    out = np.array(slab, dtype=np.float64, copy=True)
    assert out.shape == (as_rows(rows).shape[0], n)
    out[diagonal_mask(rows, n)] = diagonal
    if dead is not None:
        out[dead_mask(rows, n)] = dead
    return np.ascontiguousarray(out)


def pairs_read(rows, slab, n, read="live"):
    """(s, t, v) of the elements a flat pass reads, row-major, s <= t (s == t only under read="all": a diagonal taken for a pair)."""
    rows = as_rows(rows)
    slab = np.asarray(slab, dtype=np.float64)
    assert slab.shape == (rows.shape[0], n) and read in ("live", "all")
    mask = live_mask(rows, n) if read == "live" else np.ones((rows.shape[0], n), dtype=bool)
    k, g = np.nonzero(mask)
    q = rows[k]
    return np.minimum(q, g), np.maximum(q, g), slab[k, g]


def query_sets(n, with_all):
    """The query sets of a shape: the first genome, the last, two adjacent ones, every second one, all but one, and all of them."""
    sets = {"first": [0], "last": [n - 1], "adjacent": [n // 2 - 1, n // 2] if n > 2 else [0, 1], "every second": list(range(0, n, 2)),
            "all but one": [g for g in range(n) if g != n // 3]}
    if with_all:
        sets["all"] = list(range(n))
    return {name: as_rows(rows) for name, rows in sets.items()}


def best_value(as_distance):
    """What comes first in every list of a nearest fill, and passes every threshold of an edge or components fill."""
    return -np.inf if as_distance else np.inf


# ---- seeds that satisfy only the contract -------------------------------------------------------------------------------------
def labelling_seed(n, rows, seed, classes=None):
    """A random valid labelling: the old genomes dealt into classes, a label the smallest member of its class; every query genome
    labels itself."""
    rng = np.random.default_rng(seed)
    query = query_mask(rows, n)
    old = np.flatnonzero(~query)
    labels = np.arange(n, dtype=np.int32)
    if old.shape[0]:
        classes = max(1, old.shape[0] // 4) if classes is None else classes
        dealt = rng.integers(0, classes, size=old.shape[0])
        for c in np.unique(dealt):
            members = old[dealt == c]
            labels[members] = members.min()
    assert (labels <= np.arange(n)).all() and (labels[labels] == labels).all() and (labels[query] == np.flatnonzero(query)).all()
    return labels


def forest_seed(n, rows, seed, p_root=0.2, micros=None):
    """A random spanning forest of the old genomes, (src, tgt, val) with src < tgt in a shuffled order: every old genome but the first
    of a random order is, with probability 1 - p_root, joined to a random earlier one.  Values: millionths from ``micros`` (default: any)."""
    rng = np.random.default_rng(seed)
    old = np.flatnonzero(~query_mask(rows, n))
    order = rng.permutation(old)
    src, tgt = [], []
    for i in range(1, order.shape[0]):
        if rng.random() >= p_root:
            a, b = int(order[i]), int(order[rng.integers(0, i)])
            src.append(min(a, b))
            tgt.append(max(a, b))
    count = len(src)
    micro = rng.integers(0, MILLION + 1, size=count) if micros is None else rng.choice(np.asarray(micros, dtype=np.int64), size=count)
    shuffle = rng.permutation(count)
    return (np.asarray(src, dtype=np.int32)[shuffle], np.asarray(tgt, dtype=np.int32)[shuffle], tri.of_micros(micro)[shuffle])


def order_key(values, as_distance):
    """u64 keys whose unsigned order is the order of a nearest fill's lists: the f64 total order on distances, its complement on
    similarities."""
    key = tri.total_order_key(values)
    return key if as_distance else ~key


def finite_pool(seed):
    return np.unique(tri.finite_doubles(40, seed).view(np.uint64)).view(np.float64)


def lists_seed(n, rows, k_seed, seed, as_distance=True, pool=None):
    """Random stored lists (nbr int32[n][k_seed], val f64[n][k_seed]): each old genome's row holds k_seed distinct other old genomes
    with values from ``pool`` (default: the finite-doubles pool), strictly ascending in (order, then index).  The query genomes' rows hold
    what the fill must ignore: -7 and NaN."""
    rng = np.random.default_rng(seed)
    pool = finite_pool(seed) if pool is None else np.asarray(pool, dtype=np.float64)
    query = query_mask(rows, n)
    old = np.flatnonzero(~query)
    assert 0 <= k_seed <= max(old.shape[0] - 1, 0)
    nbr = np.full((n, k_seed), -7, dtype=np.int32)
    val = np.full((n, k_seed), np.nan, dtype=np.float64)
    for g in old.tolist():
        others = rng.choice(old[old != g], size=k_seed, replace=False)
        values = pool[rng.integers(0, pool.shape[0], size=k_seed)]
        order = np.lexsort((others, order_key(values, as_distance)))
        nbr[g], val[g] = others[order], values[order]
    return nbr, val


# ---- references ---------------------------------------------------------------------------------------------------------------
def edges(rows, slab, n, threshold, as_distance=True, read="live"):
    """(src, tgt, val) of the pairs read that pass (non-strict, as the edge fill), sorted by (t, s)."""
    s, t, v = pairs_read(rows, slab, n, read)
    keep = tri.passing(v, threshold, as_distance, strict=False)
    s, t, v = s[keep], t[keep], v[keep]
    order = np.lexsort((s, t))
    return s[order].astype(np.int32), t[order].astype(np.int32), v[order]


def united(labels, s, t):
    """The labelling (the smallest member of every class) of a valid labelling united along the pairs (s, t): every pair hooks the
    larger of its two labels under the smaller, labels are flattened, until nothing changes."""
    labels = np.asarray(labels, dtype=np.int64).copy()
    while True:
        ls, lt = labels[s], labels[t]
        low = np.minimum(ls, lt)
        before = labels.copy()
        np.minimum.at(labels, ls, low)
        np.minimum.at(labels, lt, low)
        while True:
            flat = labels[labels]
            if np.array_equal(flat, labels):
                break
            labels = flat
        if np.array_equal(labels, before):
            return labels.astype(np.int32)


def components(seed_labels, rows, slab, n, threshold, as_distance=True, strict=True, read="live"):
    """(labels, the call's passing count): the seed labelling (None: every genome its own class) united along the passing pairs read."""
    s, t, v = pairs_read(rows, slab, n, read)
    keep = tri.passing(v, threshold, as_distance, strict)
    start = np.arange(n, dtype=np.int32) if seed_labels is None else seed_labels
    return united(start, s[keep], t[keep]), int(keep.sum())


def millionths(values):
    """The millionths of values, and which are none in [0, 1] (the tree fill's check: -0.0 is the millionth 0)."""
    values = np.asarray(values, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.rint(values * 1.0e6)
        good = (k >= 0.0) & (k <= 1.0e6) & (k / 1000000.0 == values)
    return np.where(good, k, 0.0).astype(np.int64), ~good


def tree(seed, rows, slab, n, as_distance=True, read="live"):
    """(src, tgt, val) of the tree Kruskal's algorithm accepts over the seed edges ((src, tgt, val) or None) and the pairs read, taken in
    the project's order (micro on distances, 10^6 - micro on similarities; then t; then s), in that order.  ``Refused`` when an element
    read is no millionth in [0, 1]."""
    s, t, v = pairs_read(rows, slab, n, read)
    micro, bad = millionths(v)
    if bad.any():
        raise Refused(int(bad.sum()))
    if seed is not None and len(seed[0]):
        s = np.concatenate([np.asarray(seed[0], dtype=np.int64), s])
        t = np.concatenate([np.asarray(seed[1], dtype=np.int64), t])
        micro = np.concatenate([tri.micros_of(seed[2]), micro])
    order = np.lexsort((s, t, micro if as_distance else MILLION - micro))
    forest, kept = tri._UnionFind(n), []
    for e, a, b in zip(order.tolist(), s[order].tolist(), t[order].tolist()):
        if a != b and forest.union(a, b):
            kept.append(e)
            if len(kept) == n - 1:
                break
    kept = np.array(kept, dtype=np.int64)
    return s[kept].astype(np.int32), t[kept].astype(np.int32), tri.of_micros(micro[kept])


def nearest(seed, rows, slab, n, k, as_distance=True, read="live"):
    """(nbr int32[n][kk], bits of val u64[n][kk]), kk = min(k, n - 1).  An old genome: the best kk of the seed's first
    min(k_seed, kk, N_old - 1) entries ((nbr, val) or None) and the candidates (slab[k][g], rows[k]).  A query genome: the best kk of its
    row without the diagonal (read="all": with it, as the candidate that names the genome itself).  Best: by (order_key, then index)."""
    rows = as_rows(rows)
    slab = np.asarray(slab, dtype=np.float64)
    query = query_mask(rows, n)
    n_old = n - rows.shape[0]
    kk = max(min(k, n - 1), 0)
    keys = order_key(slab, as_distance)
    bits = np.ascontiguousarray(slab).view(np.uint64)
    ks = 0 if seed is None else min(seed[0].shape[1], kk, max(n_old - 1, 0))
    nbr = np.empty((n, kk), dtype=np.int32)
    val = np.empty((n, kk), dtype=np.uint64)
    row_of = {int(q): i for i, q in enumerate(rows.tolist())}
    for g in range(n):
        if query[g]:
            i = row_of[g]
            others = np.arange(n) if read == "all" else np.concatenate([np.arange(g), np.arange(g + 1, n)])
            cand_key, cand_bits = keys[i, others], bits[i, others]
        else:
            others, cand_key, cand_bits = rows, keys[:, g], bits[:, g]
            if ks:
                stored = np.ascontiguousarray(seed[1][g, :ks], dtype=np.float64)
                others = np.concatenate([np.asarray(seed[0][g, :ks], dtype=np.int64), others])
                cand_key = np.concatenate([order_key(stored, as_distance), cand_key])
                cand_bits = np.concatenate([stored.view(np.uint64), cand_bits])
        order = np.lexsort((others, cand_key))[:kk]
        assert order.shape[0] == kk, "fewer candidates than the list is long"
        nbr[g], val[g] = others[order], cand_bits[order]
    return nbr, val


# ---- the triangular references' results as seeds and merged results (the grow invariant) ----------------------------------------
def old_block(triangle, n, rows):
    """(old genomes ascending, the value triangle of the old genomes alone)."""
    old = np.flatnonzero(~query_mask(rows, n))
    full = tri.square(np.asarray(triangle, dtype=np.float64), n)
    sub = full[np.ix_(old, old)]
    t, s = np.tril_indices(old.shape[0], k=-1)
    return old, np.ascontiguousarray(sub[t, s])


def merged_edges(old_edges, old, new_edges):
    """A stored edge list of the old block, re-indexed through ``old``, merged with the call's: sorted by (t, s)."""
    s = np.concatenate([old[old_edges[0]], np.asarray(new_edges[0], dtype=np.int64)])
    t = np.concatenate([old[old_edges[1]], np.asarray(new_edges[1], dtype=np.int64)])
    v = np.concatenate([old_edges[2], new_edges[2]])
    order = np.lexsort((s, t))
    return s[order].astype(np.int32), t[order].astype(np.int32), v[order]


# ---- the inputs of tests/rows_values_driver.py (tests/test_rows_values_host.py shows that the poison bites on every one of them) ----
FLAT_SHAPES = (63, 64, 65, 511, 512, 513)         # odd n: a thread's odd element across a row end; n < 512: a stride skips rows; 512 / 513 flip the carry
WIDE_SHAPE = (4099, (0, 2049, 4098))              # a chunk lies inside one row: 3 rows of 4,099 are just above three chunks
NAN = float("nan")


class FlatInput:
    """One input of the flat passes: a query set, a slab poisoned for the edge and components fills (the value that passes every
    threshold in the diagonal and the dead copies), the same slab poisoned with NaN for the tree fill (None: values the tree refuses),
    thresholds at and between its values, and contract-only seeds."""

    def __init__(self, label, n, rows, as_distance, base, thresholds, for_tree, seed, tie_micros=None):
        self.label, self.n, self.rows, self.as_distance, self.thresholds = label, n, as_rows(rows), as_distance, tuple(float(x) for x in thresholds)
        best = best_value(as_distance)
        self.slab = poisoned(base, rows, n, best, best)
        self.tree_slab = poisoned(base, rows, n, NAN, NAN) if for_tree else None
        self.labels = labelling_seed(n, rows, seed)
        self.forest = forest_seed(n, rows, seed + 1, micros=tie_micros)


TIE_THRESHOLDS = {True: (0.0, 5e-7, 1e-6, 0.5), False: (1.0, 0.9999995, 0.999999, 0.5)}       # at and between the smallest distances / the largest similarities


def quantile_thresholds(base, rows, n, as_distance, share=0.03):
    """A threshold AT a live value that about ``share`` of the live values pass, and one between it and the next millionth."""
    live = np.sort(base[live_mask(rows, n)])
    if not as_distance:
        live = live[::-1]
    at = float(live[int(share * live.shape[0])])
    return (at, at + 5e-7 if as_distance else at - 5e-7)


def finite_thresholds(base, rows, n):
    """A present value with its two neighbours in the doubles, and the two zeros."""
    present = np.unique(base[live_mask(rows, n)])
    v = float(present[present.shape[0] // 2])
    return (0.0, -0.0, float(np.nextafter(v, np.inf)), float(np.nextafter(v, -np.inf)), v)


def direct_slab(m, n, kind, seed):
    """A rows slab made without its triangle (for shapes whose triangle would be large): every element its own value.  The flat passes
    read one copy of a pair only, so nothing asks for symmetry."""
    rng = np.random.default_rng(seed)
    if kind == "ramp":
        return tri.of_micros(np.arange(m * n, dtype=np.int64) * tri.RAMP_STRIDE % (MILLION + 1)).reshape(m, n)
    if kind == "tie_set":
        return tri.of_micros(rng.choice(np.array(tri.TIE_MICROS, dtype=np.int64), size=(m, n)))
    if kind == "two_valued":
        return np.where(rng.random((m, n)) < 0.5, 0.0, 1.0 / 1000000.0)
    assert kind == "finite"
    pool = finite_pool(seed)
    return pool[rng.integers(0, pool.shape[0], size=(m, n))].copy()


def flat_inputs(n, query_names=None):
    """The inputs of the flat passes at n genomes: every query set x (ramp, tie_set, two_valued, finite doubles) x both directions."""
    sets = query_sets(n, with_all=n <= 65)
    triangles = {"ramp": tri.ramp(n), "tie_set": tri.tie_set(n, 200 + n), "two_valued": tri.two_valued(n, 0.5, 300 + n), "finite": tri.finite_doubles(n, 400 + n)}
    for q, (qname, rows) in enumerate(sets.items()):
        if query_names is not None and qname not in query_names:
            continue
        for v, (vname, triangle) in enumerate(triangles.items()):
            base = rows_of(triangle, n, rows)
            for as_distance in (True, False):
                if vname == "ramp":
                    thresholds = quantile_thresholds(base, rows, n, as_distance)
                elif vname == "tie_set":
                    thresholds = TIE_THRESHOLDS[as_distance]
                elif vname == "two_valued":
                    thresholds = (0.0, 1e-6, 5e-7)
                else:
                    thresholds = finite_thresholds(base, rows, n)
                yield FlatInput((n, qname, vname, as_distance), n, rows, as_distance, base, thresholds, vname != "finite", 1000 * n + 10 * q + v,
                                tie_micros=None if vname == "ramp" else tri.TIE_MICROS)


def wide_inputs():
    n, rows = WIDE_SHAPE
    rows = as_rows(rows)
    for v, kind in enumerate(("ramp", "tie_set", "two_valued", "finite")):
        base = direct_slab(rows.shape[0], n, kind, 500 + v)
        for as_distance in (True, False):
            if kind == "ramp":
                thresholds = quantile_thresholds(base, rows, n, as_distance)
            elif kind == "tie_set":
                thresholds = TIE_THRESHOLDS[as_distance]
            elif kind == "two_valued":
                thresholds = (0.0, 1e-6, 5e-7)
            else:
                thresholds = finite_thresholds(base, rows, n)
            yield FlatInput((n, "first, middle, last", kind, as_distance), n, rows, as_distance, base, thresholds, False, 7000 + v)


def tiny_inputs():
    """n = 2 and 3: every genome a query, then each genome alone, then (n = 3) each two -- where the odd element of a thread's pair lies
    across a row end and is live --; at n = 3 every assignment of three millionths to the pairs."""
    import itertools
    micros = (0, 500000, 1000000)
    for n, patterns in ((2, [(a,) for a in micros]), (3, list(itertools.product(micros, repeat=3)))):
        for rows in [list(range(n))] + [[g] for g in range(n)] + ([[0, 1], [0, 2], [1, 2]] if n == 3 else []):
            for pattern in patterns:
                base = rows_of(tri.of_micros(pattern), n, rows)
                for as_distance in (True, False):
                    yield FlatInput((n, tuple(rows), pattern, as_distance), n, rows, as_distance, base, (0.0, 0.5, 0.75), True, 17,
                                    tie_micros=micros)


class NearestInput:
    """One input of the nearest fill: a symmetric slab whose diagonal holds the best possible value, K, and a contract-only seed."""

    def __init__(self, label, n, rows, as_distance, triangle, k, seed):
        self.label, self.n, self.rows, self.as_distance, self.k, self.seed = label, n, as_rows(rows), as_distance, k, seed
        self.slab = poisoned(rows_of(triangle, n, rows), rows, n, best_value(as_distance))


def nearest_query_sets(n):
    """Query sets of 1, 63, 64, 65 (and n) genomes where they fit: blocks that straddle column 16 (a wave's first) and column 64 (a
    workgroup's first), single genomes on either side of both, and every second genome."""
    sets = {}
    for g in (0, 15, 16, 63, 64, n - 1):
        if 0 <= g < n:
            sets[f"genome {g}"] = [g]
    for m, first in ((63, 10), (64, 40), (65, 32), (63, 1), (64, 1)):
        if first + m <= n:
            sets[f"{m} from {first}"] = list(range(first, first + m))
    if len(range(0, n, 2)) in (63, 64, 65):
        sets["every second"] = list(range(0, n, 2))
    sets["all"] = list(range(n))                                             # m = n: an empty seed
    return {name: as_rows(rows) for name, rows in sets.items()}


def nearest_ks(n):
    return sorted({k for k in (1, 5, 63, 64, n - 1, n) if 1 <= k <= 64})


def seed_k(n, m, k, above):
    """k_seed of a contract-only seed: what the fill needs, min(kk, N_old - 1), or more where the old genomes allow (columns beyond kk
    are cut)."""
    n_old, kk = n - m, min(k, n - 1)
    need = max(min(kk, n_old - 1), 0)
    return min(need + 3, max(n_old - 1, 0)) if above else need


def nearest_inputs(n):
    """The inputs of the nearest fill at n genomes: every query set x (finite doubles, tie_set, all-distinct) x K x both directions x
    (k_seed as needed, k_seed above it); with tie_set values the seed draws from the same seven values, so a new candidate ties stored
    entries of smaller and of larger index, and one finite-doubles seed holds only the two zeros and their neighbours."""
    zeros = np.array([-0.0, 0.0, 5e-324, -5e-324])
    triangles = {"finite": tri.finite_doubles(n, 600 + n), "tie_set": tri.tie_set(n, 700 + n), "distinct": tri.ramp(n)}
    for q, (qname, rows) in enumerate(nearest_query_sets(n).items()):
        m = rows.shape[0]
        for v, (vname, triangle) in enumerate(triangles.items()):
            for i, k in enumerate(nearest_ks(n)):
                for as_distance in (True, False):
                    above = (q + v + i) % 2 == 1
                    k_seed = seed_k(n, m, k, above)
                    pools = {"finite": zeros if (q + i) % 3 == 0 else None, "tie_set": tri.of_micros(tri.TIE_MICROS), "distinct": tri.of_micros(np.arange(0, MILLION, 37))}
                    seed = lists_seed(n, rows, k_seed, 10000 * n + 100 * q + 10 * v + i, as_distance, pools[vname]) if n - m > 1 else None
                    yield NearestInput((n, qname, vname, k, as_distance, k_seed), n, rows, as_distance, triangle, k, seed)
