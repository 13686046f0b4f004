"""Value triangles for the slab fills and the plain statements of what each fill makes of one (no GPU, no use of the library).

A value triangle is what a triangular slab walk fills: ``n (n - 1) / 2`` doubles, target-major -- element ``t (t - 1) / 2 + s`` is the
pair ``(s, t)``, ``s < t``.  ``Context`` fills it from genomes; ``hip.set_slab_values`` (the test-hooks twin) puts any triangle in its
place, so the kernels behind ``fill_edges`` / ``_components`` / ``_nearest`` / ``_tree`` / ``_between`` / ``_affinity`` can be run on
values no genome collection produces: random ties, elements that all differ, and values the fills must refuse.

The generators are seeded; the references are numpy and pure Python over int64 millionths and f64 bit patterns.
tests/test_slab_values_host.py holds every reference to the host statements the project already trusts
(``matrix.SingleLinkageTree`` / ``SparseEdges`` / ``NearestNeighbors`` / ``GroupLinkage`` / ``GroupAffinity`` ``.from_dense``);
tests/slab_values_driver.py holds the kernels to the references."""

import numpy as np

MILLION = 10 ** 6
EMPTY_LO, EMPTY_HI = 2 ** 31 - 1, -1
TIE_MICROS = (0, 1, 499999, 500000, 500001, 999999, 1000000)
RAMP_STRIDE = 7919        # prime; coprime to 10^6 and to 1000001 = 101 * 9901: i -> i * stride mod 1000001 is a bijection of the millionths
BAD_VALUES = (float("nan"), float("inf"), -1e-6, 1.000001, 0.1234565, 5e-7)


def n_pairs(n):
    return n * (n - 1) // 2


def pair_index(s, t):
    """Where the pair (s, t), s < t, lies in a triangle."""
    assert 0 <= s < t
    return t * (t - 1) // 2 + s


def pair_ends(n):
    """(s, t) of every element of a triangle of n genomes, in its order."""
    t, s = np.tril_indices(n, k=-1)
    return s.astype(np.int64), t.astype(np.int64)


def square(values, n, diagonal=0.0):
    """The symmetric n x n array of a triangle."""
    values = np.asarray(values)
    assert values.shape == (n_pairs(n),)
    s, t = pair_ends(n)
    out = np.full((n, n), diagonal, dtype=values.dtype)
    out[t, s] = values
    out[s, t] = values
    return out


def of_micros(micro):
    """Millionths as the doubles a fill delivers: k / 1000000.0."""
    return np.asarray(micro, dtype=np.int64).astype(np.float64) / 1000000.0


def micros_of(values):
    """The millionths of a triangle of valid values (-0.0 is the millionth 0)."""
    values = np.asarray(values, dtype=np.float64)
    k = np.rint(values * 1.0e6)
    assert ((k >= 0.0) & (k <= 1.0e6)).all() and np.array_equal(k / 1000000.0, values), "no millionths in [0, 1]"
    return k.astype(np.int64)


# ---- generators -------------------------------------------------------------------------------------------------------
def two_valued(n, p, seed):
    """0.0 with probability p, else one millionth."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n_pairs(n)) < p, 0.0, 1.0 / 1000000.0)


def rescaled(values, low_micro, high_micro):
    """A two_valued triangle on two other millionths: its zeros become low_micro, the rest high_micro."""
    return of_micros(np.where(np.asarray(values) == 0.0, low_micro, high_micro))


def tie_set(n, seed):
    rng = np.random.default_rng(seed)
    return of_micros(rng.choice(np.array(TIE_MICROS, dtype=np.int64), size=n_pairs(n)))


def spread(n, seed):
    rng = np.random.default_rng(seed)
    return of_micros(rng.integers(0, MILLION + 1, size=n_pairs(n)))


def ramp(n):
    """Element i holds the millionth (i * RAMP_STRIDE) % 1000001: any 1,000,001 consecutive elements all differ -- a whole triangle up
    to n = 1,414, and every row of any triangle the fills take in one piece -- and so do neighbouring rows."""
    return of_micros(np.arange(n_pairs(n), dtype=np.int64) * RAMP_STRIDE % (MILLION + 1))


def finite_doubles(n, seed):
    """For the fills that take any finite double (nearest, edges, components): negatives, both zeros, subnormals, values above 1,
    and pairs one ulp apart, drawn from a small pool so that exact ties are frequent as well."""
    rng = np.random.default_rng(seed)
    base = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-310, -2.5e-310, 2.2250738585072014e-308, 1e-6, 0.25, 0.5, 0.999999, 1.0, 1.5, 3.0,
                     1e300, -1e-6, -0.5, -1.0, -2.0, -1e300, 1.7976931348623157e308, -1.7976931348623157e308])
    with np.errstate(over="ignore"):                                        # (beyond the largest double: dropped below)
        pool = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf), rng.standard_normal(8)])
    pool = pool[np.isfinite(pool)]
    return pool[rng.integers(0, pool.shape[0], size=n_pairs(n))].copy()


def with_bad(values, positions):
    """A copy with values the tree, between and affinity fills must refuse at ``positions``: NaN, +inf, -1e-6, 1.000001, 0.1234565 and
    5e-7, in turn."""
    out = np.array(values, dtype=np.float64, copy=True)
    for i, at in enumerate(positions):
        out[at] = BAD_VALUES[i % len(BAD_VALUES)]
    return out


def total_order_key(values):
    """u64 keys whose unsigned order is the f64 total order on finite doubles: negatives before -0.0 before +0.0 before positives."""
    u = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    negative = (u >> np.uint64(63)).astype(bool)
    return np.where(negative, ~u, u ^ np.uint64(1 << 63))


# ---- references --------------------------------------------------------------------------------------------------------
class _UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        parent = self.parent
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra == rb:
            return False
        self.parent[max(ra, rb)] = min(ra, rb)
        return True

    def labels(self):
        return np.array([self.find(g) for g in range(len(self.parent))], dtype=np.int32)      # the smaller root wins: the smallest member


def kruskal(values, n, as_distance=True):
    """(src, tgt, val) of the tree Kruskal's algorithm accepts when it takes the pairs in the order (micro on distances, 10^6 - micro on
    similarities; then t; then s), in that order; val = micro / 1000000.0."""
    micro = micros_of(values)
    s, t = pair_ends(n)
    order = np.lexsort((s, t, micro if as_distance else MILLION - micro))
    forest, kept = _UnionFind(n), []
    for e, a, b in zip(order.tolist(), s[order].tolist(), t[order].tolist()):
        if forest.union(a, b):
            kept.append(e)
            if len(kept) == n - 1:
                break
    kept = np.array(kept, dtype=np.int64)
    return s[kept].astype(np.int32), t[kept].astype(np.int32), of_micros(micro[kept])


def passing(values, threshold, as_distance=True, strict=False):
    """Which elements pass a threshold: plain f64 compares (the two zeros are equal)."""
    values = np.asarray(values, dtype=np.float64)
    if as_distance:
        return values < threshold if strict else values <= threshold
    return values > threshold if strict else values >= threshold


def edge_list(values, n, threshold, as_distance=True, strict=False):
    """(src, tgt, val) of the passing pairs sorted by (t, s) -- the triangle's own order.  The edge fill is the non-strict one."""
    s, t = pair_ends(n)
    keep = np.flatnonzero(passing(values, threshold, as_distance, strict))
    return s[keep].astype(np.int32), t[keep].astype(np.int32), np.asarray(values, dtype=np.float64)[keep]


def components(values, n, threshold, as_distance=True, strict=True):
    """(labels, number of passing pairs): labels[g] = the smallest member of g's component of the graph of passing pairs."""
    s, t = pair_ends(n)
    keep = np.flatnonzero(passing(values, threshold, as_distance, strict))
    forest = _UnionFind(n)
    for a, b in zip(s[keep].tolist(), t[keep].tolist()):
        forest.union(a, b)
    return forest.labels(), int(keep.shape[0])


def nearest(values, n, k, as_distance=True):
    """(nbr, bits of val) [n, kk]: every genome's kk = min(k, n - 1) best others under (f64 total order, then index); on similarities
    the total order complemented (the largest first, +0.0 before -0.0), then index."""
    kk = max(min(k, n - 1), 0)
    keys = square(total_order_key(values), n, diagonal=np.uint64(0))
    bits = square(np.ascontiguousarray(values, dtype=np.float64).view(np.uint64), n, diagonal=np.uint64(0))
    if not as_distance:
        keys = ~keys
    nbr = np.empty((n, kk), dtype=np.int32)
    val = np.empty((n, kk), dtype=np.uint64)
    for g in range(n):
        others = np.concatenate([np.arange(g), np.arange(g + 1, n)])
        order = others[np.lexsort((others, keys[g, others]))][:kk]
        nbr[g], val[g] = order, bits[g, order]
    return nbr, val


def group_sizes(group, n_groups):
    return np.bincount(np.asarray(group, dtype=np.int64), minlength=n_groups).astype(np.int64)


def between(values, n, group, n_groups, as_distance=True):
    """(sum, count, lo, hi) [G, G] of the millionths between every two groups (within a group on the diagonal), symmetric; an entry
    without a pair reads 0, 0, 2^31 - 1, -1.  ``values`` are distances; as_distance=False: that table inverted."""
    micro = micros_of(values)
    group = np.asarray(group, dtype=np.int64)
    s, t = pair_ends(n)
    a, b = np.minimum(group[s], group[t]), np.maximum(group[s], group[t])
    flat = a * n_groups + b
    gg = n_groups * n_groups
    count =np.bincount(flat, minlength=gg).astype(np.int64)
    total = np.zeros(gg, dtype=np.int64)
    np.add.at(total, flat, micro)
    lo = np.full(gg, EMPTY_LO, dtype=np.int64)
    hi = np.full(gg, EMPTY_HI, dtype=np.int64)
    np.minimum.at(lo, flat, micro)
    np.maximum.at(hi, flat, micro)
    out = []
    for arr in (total, count, lo, hi):
        arr = arr.reshape(n_groups, n_groups)
        upper = np.triu(np.ones((n_groups, n_groups), dtype=bool))
        out.append(np.where(upper, arr, arr.T))
    total, count, lo, hi = out
    if not as_distance:
        full = count > 0
        total, lo, hi = count * MILLION - total, np.where(full, MILLION - hi, EMPTY_LO), np.where(full, MILLION - lo, EMPTY_HI)
    return total.astype(np.int64), count.astype(np.int64), lo.astype(np.int32), hi.astype(np.int32)


def affinity(values, n, group, n_groups, as_distance=True):
    """The affinity fill's dict (own_sum, own_lo, own_hi, near_group [3, n], near_sum, near_lo, near_hi, table = (sum, lo, hi) [n, G]) of
    the DISTANCES ``values``; as_distance=False: the same nearest groups, every value complemented.  Means are compared as exact
    Python-integer cross products; ties go to the smaller group index."""
    micro = square(micros_of(values), n, diagonal=0)
    group = np.asarray(group, dtype=np.int64)
    sizes = group_sizes(group, n_groups)
    onehot = np.zeros((n, n_groups), dtype=np.int64)
    onehot[np.arange(n), group] = 1
    total = micro @ onehot                                                   # the diagonal holds 0: no pair adds to a sum
    count = np.broadcast_to(sizes, (n, n_groups)).copy()
    count[np.arange(n), group] -= 1
    lo = np.full((n, n_groups), EMPTY_LO, dtype=np.int64)
    hi = np.full((n, n_groups), EMPTY_HI, dtype=np.int64)
    low, high = micro.copy(), micro.copy()
    np.fill_diagonal(low, EMPTY_LO)
    np.fill_diagonal(high, EMPTY_HI)
    for b in np.flatnonzero(sizes > 0).tolist():
        members = np.flatnonzero(group == b)
        lo[:, b], hi[:, b] = low[:, members].min(axis=1), high[:, members].max(axis=1)
    near = np.full((3, n), -1, dtype=np.int32)
    near_sum, near_lo, near_hi = np.zeros(n, dtype=np.int64), np.full(n, EMPTY_LO, dtype=np.int64), np.full(n, EMPTY_HI, dtype=np.int64)
    near_size = np.zeros(n, dtype=np.int64)
    present = np.flatnonzero(sizes > 0).tolist()
    size_of = sizes.tolist()
    for g in range(n):
        own, row = int(group[g]), total[g].tolist()
        best = -1
        for b in present:
            if b != own and (best < 0 or row[b] * size_of[best] < row[best] * size_of[b]):      # Python integers: exact
                best = b
        if best < 0:
            continue
        others = np.array([b for b in present if b != own], dtype=np.int64)
        by_lo, by_hi = int(others[np.argmin(lo[g, others])]), int(others[np.argmin(hi[g, others])])     # the first minimum: the smaller index
        near[:, g] = best, by_lo, by_hi
        near_sum[g], near_size[g], near_lo[g], near_hi[g] = row[best], size_of[best], lo[g, by_lo], hi[g, by_hi]
    rows = np.arange(n)
    own_count = count[rows, group]
    own_sum, own_lo, own_hi = total[rows, group], lo[rows, group], hi[rows, group]
    if not as_distance:
        def flipped(x_sum, x_lo, x_hi, x_count):
            full = x_count > 0
            return np.where(full, x_count * MILLION - x_sum, 0), np.where(full, MILLION - x_hi, EMPTY_LO), np.where(full, MILLION - x_lo, EMPTY_HI)
        own_sum, own_lo, own_hi = flipped(own_sum, own_lo, own_hi, own_count)
        total, lo, hi = flipped(total, lo, hi, count)
        some = near[0] >= 0
        near_sum = np.where(some, near_size * MILLION - near_sum, 0)
        near_lo, near_hi = np.where(some, MILLION - near_lo, EMPTY_LO), np.where(some, MILLION - near_hi, EMPTY_HI)
    return dict(own_sum=own_sum.astype(np.int64), own_lo=own_lo.astype(np.int32), own_hi=own_hi.astype(np.int32), near_group=near,
                near_sum=near_sum.astype(np.int64), near_lo=near_lo.astype(np.int32), near_hi=near_hi.astype(np.int32),
                table=(total.astype(np.int64), lo.astype(np.int32), hi.astype(np.int32)))


def affinity_goff(group, n_groups):
    """goff[G + 1] of a labelling: each group's run among the genomes sorted by (group, index)."""
    return np.concatenate([[0], np.cumsum(group_sizes(group, n_groups))]).astype(np.int32)
