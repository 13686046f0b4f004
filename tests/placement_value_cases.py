"""Shared by tests/test_placement_host.py (CPU) and tests/placement_values_driver.py (GPU): the injected inputs of the rows form of the
affinity fill, and the plain statement of its definition.

An input is a symmetric matrix of millionths over n genomes, labels in [-1, G) and query rows; its rows slab is the queries' rows of the
matrix with every element no pass may read POISONED (NaN): the diagonal and every column of an unlabelled genome.  The expected result
is ``GroupPlacement.from_dense`` of the matrix, which test_placement_host.py holds to ``loops`` below -- a triple loop over python ints."""

import numpy as np

MILLION = 1000000
EMPTY_LO, EMPTY_HI = 2**31 - 1, -1
SHAPES = (2, 3, 63, 64, 65, 255, 256, 257, 513)
GROUPS = (1, 3, 64, 65, 2048)
WIDE = 4300                                  # 4,299 values of 10^6 in one entry: a sum above 2^32
BAD_VALUES = (float("nan"), float(np.nextafter(1.0, 2.0)), 0.1234567)     # NaN, 1 + ulp, no millionth


class Input:
    def __init__(self, tag, micro, label, n_groups, rows):
        self.tag, self.micro, self.n_groups = tag, micro, int(n_groups)
        self.n = micro.shape[0]
        self.label = np.asarray(label, dtype=np.int32)
        self.rows = np.asarray(sorted(set(int(r) for r in rows)), dtype=np.int32)
        self.names = [f"g{i:04d}" for i in range(self.n)]
        self.groups = [[self.names[i] for i in np.flatnonzero(self.label == b)] for b in range(self.n_groups)]
        self.queries = [self.names[r] for r in self.rows]

    def values(self):
        """The symmetric matrix as doubles: exact millionths, the diagonal 0."""
        return self.micro.astype(np.float64) / 1.0e6

    def matrix(self, as_distance=True):
        from phamclust_amd.symmatrix import _square_matrix
        values = self.values()
        if not as_distance:
            values = (MILLION - self.micro).astype(np.float64) / 1.0e6
            np.fill_diagonal(values, 1.0)
        return _square_matrix(self.names, values, as_distance)

    def slab(self, negative_zero=True):
        """f64[m][n] as the rows walk lays it out, poisoned where nothing may read; every other 0 as -0.0."""
        slab = self.values()[self.rows].copy()
        if negative_zero:
            zeros = np.argwhere(slab == 0.0)
            slab[tuple(zeros[::2].T)] = -0.0
        slab[:, self.label < 0] = np.nan
        slab[np.arange(self.rows.shape[0]), self.rows] = np.nan
        return slab

    def expected(self):
        from phamclust_amd.matrix import GroupPlacement
        return GroupPlacement.from_dense(self.matrix(), self.groups, self.queries)


def symmetric(n, seed, pool=None):
    """int64[n][n], symmetric, diagonal 0: uniform millionths, or drawn from ``pool``."""
    rng = np.random.default_rng(seed)
    upper = rng.integers(0, MILLION + 1, size=(n, n)) if pool is None else rng.choice(np.asarray(pool, dtype=np.int64), size=(n, n))
    upper = np.triu(upper, 1)
    return (upper + upper.T).astype(np.int64)


def labels(kind, n, n_groups, seed=0):
    g = np.arange(n, dtype=np.int64)
    if kind == "runs":                       # runs of 70 consecutive same-group columns: whole waves of one group
        label = (g // 70) % n_groups
    elif kind == "alternating":              # neighbours differ wherever G > 1: the atomic path
        label = g % n_groups
    else:                                    # scattered: most of a large G's groups stay empty
        label = (g * 37 + seed) % n_groups
    return label.astype(np.int32)


def query_rows(n):
    """Both ends, two adjacent pairs (one inside one 64-column block), and a few more."""
    return sorted({0, 1, n - 1, n - 2, n // 2, n // 2 + 1} & set(range(n)) | set(range(5, n, 97)))


def inputs(n):
    """The inputs of shape n: every G of GROUPS under the three labellings; -1 labels on a query, on an old genome inside a run and
    on the neighbour of a diagonal; values uniform, from a pool of few values (ties, the ends 0 and 10^6), and constant (every
    criterion ties between all groups: the smaller index wins)."""
    out = []
    rows = query_rows(n)
    for k, n_groups in enumerate(GROUPS):
        for kind in ("runs", "alternating", "scattered"):
            for pool_tag, pool in (("uniform", None), ("few", (0, 1, 499999, 500000, 500001, MILLION)), ("constant", (250000,))):
                if pool_tag != "uniform" and kind == "scattered" and n_groups not in (3, 2048):
                    continue
                label = labels(kind, n, n_groups, seed=k)
                for g in {1, n // 2 + 2, n - 2, 40, 41} & set(range(n)):     # query 1 (and n - 2) unlabelled; old genomes inside a run
                    if n > 3 or g == 1:
                        label[g] = -1
                out.append(Input(f"n{n}_G{n_groups}_{kind}_{pool_tag}", symmetric(n, 1000 * n + 10 * k + len(out), pool), label, n_groups, rows))
    return out


def wide_input():
    micro = np.full((WIDE, WIDE), MILLION, dtype=np.int64)
    np.fill_diagonal(micro, 0)
    return Input("wide_sum", micro, np.zeros(WIDE, dtype=np.int32), 1, [0, WIDE - 1])


def loops(micro, label, n_groups, rows):
    """The definition by plain loops over python ints: per query the table rows, own, the three nearest groups and their values; the gain
    per genome.  Returns dict of lists."""
    n = len(label)
    micro, label, rows = micro.tolist(), [int(x) for x in label], [int(r) for r in rows]
    is_query = [g in set(rows) for g in range(n)]
    size = [sum(1 for x in label if x == b) for b in range(n_groups)]
    out = dict(tab_sum=[], tab_lo=[], tab_hi=[], own=[], near_group=[[], [], []], near_sum=[], near_lo=[], near_hi=[])
    for q in rows:
        entries = []
        for b in range(n_groups):
            vals = [micro[q][x] for x in range(n) if x != q and label[x] == b]
            entries.append((sum(vals), min(vals), max(vals)) if vals else (0, EMPTY_LO, EMPTY_HI))
        out["tab_sum"].append([e[0] for e in entries]); out["tab_lo"].append([e[1] for e in entries]); out["tab_hi"].append([e[2] for e in entries])
        out["own"].append(entries[label[q]] if label[q] >= 0 else (0, EMPTY_LO, EMPTY_HI))
        cand = [b for b in range(n_groups) if b != label[q] and size[b] > 0]
        if not cand:
            for k in range(3):
                out["near_group"][k].append(-1)
            out["near_sum"].append(0); out["near_lo"].append(EMPTY_LO); out["near_hi"].append(EMPTY_HI)
            continue
        best = cand[0]
        for b in cand[1:]:                   # the mean in integers: sum_b * size_best < sum_best * size_b
            if entries[b][0] * size[best] < entries[best][0] * size[b]:
                best = b
        by_lo = min(cand, key=lambda b: (entries[b][1], b))
        by_hi = min(cand, key=lambda b: (entries[b][2], b))
        for k, b in enumerate((best, by_lo, by_hi)):
            out["near_group"][k].append(b)
        out["near_sum"].append(entries[best][0]); out["near_lo"].append(entries[by_lo][1]); out["near_hi"].append(entries[by_hi][2])
    gain = []
    for g in range(n):
        vals = [micro[g][x] for x in rows if not is_query[g] and label[g] >= 0 and label[x] == label[g]]
        gain.append((sum(vals), min(vals), max(vals)) if vals else (0, EMPTY_LO, EMPTY_HI))
    out["gain"] = gain
    return out


def refused_inputs():
    """(tag, Input, slab, number of refused PAIRS): a refused value in a query-old pair, in a pair of two labelled queries (both copies:
    one pair), in pairs of a labelled and an unlabelled query (read in the unlabelled one's row only, whichever is the smaller), and all of them at once."""
    n, n_groups = 130, 3
    rows = [0, 1, 40, 63, 64, 65, 100, 128, 129]
    label = labels("alternating", n, n_groups)
    label[1] = label[77] = -1
    x = Input("refused", symmetric(n, 4242), label, n_groups, rows)
    at = {int(r): k for k, r in enumerate(x.rows)}
    out = []
    for i, bad in enumerate(BAD_VALUES):
        places = {"query_old": [(at[40], 41)], "query_query": [(at[63], 64), (at[64], 63)], "labelled_unlabelled_query": [(at[1], 64), (at[1], 0)],
                  "row_end": [(at[129], 128), (at[128], 129), (at[0], n - 1), (at[129], 0)]}
        pairs = {"query_old": 1, "query_query": 1, "labelled_unlabelled_query": 2, "row_end": 2}
        everything = [p for ps in places.values() for p in ps]
        for tag, ps in list(places.items()) + [("all", everything)]:
            slab = x.slab()
            for p in ps:
                assert not np.isnan(slab[p]), (tag, p)
                slab[p] = bad
            out.append((f"{tag}_{i}", x, slab, pairs.get(tag, sum(pairs.values()))))
    return out
