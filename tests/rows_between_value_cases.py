"""Shared by tests/test_rows_between_host.py (CPU) and tests/rows_between_values_driver.py (GPU): the injected inputs of the rows form of
the between-groups fill, and the plain statement of its definition.

An input is the query rows' values, int64 millionths ``[m][n]`` (the copies of a pair of two queries agree), labels in [-1, G) and the
query rows.  Its rows slab holds those values as doubles with every DEAD element poisoned: the diagonal, the second copy of a pair of
two queries (the row of the larger genome), every column of an unlabelled genome and every row of an unlabelled query hold 0.5 -- a
value no live element holds, which would change a sum if a kernel added it -- or 2.0, which would fail the call if a kernel checked it,
alternately.  The expected table is ``loops`` below, plain loops over python ints, which test_rows_between_host.py holds to
``GroupLinkage.extended``."""

import numpy as np

MILLION = 1000000
EMPTY_LO, EMPTY_HI = 2**31 - 1, -1
POISON = (0.5, 2.0)
SEGMENT = 4096                               # PC_BETWEEN_SEGMENT: the driver asserts it is the library's


class Input:
    def __init__(self, tag, n, label, n_groups, rows, seed, pool=None):
        self.tag, self.n, self.n_groups = tag, int(n), int(n_groups)
        self.label = np.asarray(label, dtype=np.int32)
        self.rows = np.asarray(sorted(set(int(r) for r in rows)), dtype=np.int32)
        m = self.rows.shape[0]
        rng = np.random.default_rng(seed)
        if pool is None:                     # values that all differ (but the two copies of a pair of two queries), none of them 500000
            assert m * n < MILLION
            micro = rng.permutation(MILLION + 1)[: m * n + 1]
            micro = micro[micro != 500000][: m * n].reshape(m, n).astype(np.int64)
        else:
            micro = rng.choice(np.asarray(pool, dtype=np.int64), size=(m, n))
        for j in range(m):                   # a pair of two queries stands in two rows: one value
            for k in range(j):
                micro[j, self.rows[k]] = micro[k, self.rows[j]]
        assert not (micro == 500000).any()
        self.micro = micro
        self.is_query = np.zeros(n, dtype=bool)
        self.is_query[self.rows] = True

    def live(self):
        """bool[m][n]: the element is a pair of the table."""
        cols = np.arange(self.n)
        q = self.rows[:, None]
        return ((self.label[self.rows] >= 0)[:, None] & (self.label >= 0)[None, :] & (cols[None, :] != q) &
                ((cols[None, :] > q) | ~self.is_query[None, :]))

    def slab(self):
        """f64[m][n] as the rows walk lays it out: every other 0 as -0.0, every dead element poisoned."""
        slab = self.micro.astype(np.float64) / 1.0e6
        zeros = np.argwhere(slab == 0.0)
        slab[tuple(zeros[::2].T)] = -0.0
        dead = np.argwhere(~self.live())
        slab[tuple(dead[0::2].T)] = POISON[0]
        slab[tuple(dead[1::2].T)] = POISON[1]
        return slab

    def old_counts(self):
        """old[b]: the genomes labelled b that are no query rows."""
        keep = (self.label >= 0) & ~self.is_query
        return np.bincount(self.label[keep], minlength=self.n_groups).astype(np.int64)

    def table(self, as_distance=True):
        return loops(self.micro if as_distance else MILLION - self.micro, self.label, self.n_groups, self.rows)

    def contract_seed(self, seed):
        """A stored table that satisfies nothing but the contract: the partition's own counts, symmetric, 0 <= lo <= hi <= 10^6 and a sum
        in [count lo, count hi] -- of no matrix."""
        rng = np.random.default_rng(seed)
        g = self.n_groups
        old = self.old_counts()
        count = np.outer(old, old)
        np.fill_diagonal(count, old * (old - 1) // 2)
        a = rng.integers(0, MILLION + 1, size=(g, g))
        b = rng.integers(0, MILLION + 1, size=(g, g))
        lo, hi = np.triu(np.minimum(a, b)), np.triu(np.maximum(a, b))
        lo, hi = lo + np.triu(lo, 1).T, hi + np.triu(hi, 1).T
        part = np.triu(rng.integers(0, 5, size=(g, g)))
        part = part + np.triu(part, 1).T
        total = count * lo + (count * (hi - lo) * part) // 4
        full = count > 0
        return (np.where(full, total, 0).astype(np.int64), count.astype(np.int64), np.where(full, lo, EMPTY_LO).astype(np.int32),
                np.where(full, hi, EMPTY_HI).astype(np.int32))


def loops(micro, label, n_groups, rows):
    """The definition by plain loops over python ints: the table over the pairs (q, g), q a labelled query row, g labelled, g != q, and
    g > q or g no query -- ``(sum, count, lo, hi)`` as the call delivers them, symmetric."""
    g_n = int(n_groups)
    micro, label, rows = np.asarray(micro).tolist(), [int(x) for x in label], [int(r) for r in rows]
    query = set(rows)
    total = [[0] * g_n for _ in range(g_n)]
    count = [[0] * g_n for _ in range(g_n)]
    lo = [[EMPTY_LO] * g_n for _ in range(g_n)]
    hi = [[EMPTY_HI] * g_n for _ in range(g_n)]
    for k, q in enumerate(rows):
        if label[q] < 0:
            continue
        for g in range(len(label)):
            if g == q or label[g] < 0 or (g < q and g in query):
                continue
            a, b = sorted((label[q], label[g]))
            v = micro[k][g]
            for x, y in {(a, b), (b, a)}:
                total[x][y] += v
                count[x][y] += 1
                lo[x][y] = min(lo[x][y], v)
                hi[x][y] = max(hi[x][y], v)
    return (np.array(total, dtype=np.int64).reshape(g_n, g_n), np.array(count, dtype=np.int64).reshape(g_n, g_n),
            np.array(lo, dtype=np.int32).reshape(g_n, g_n), np.array(hi, dtype=np.int32).reshape(g_n, g_n))


def combined(seed, table):
    """stored (+) the pairs of the call: counts and sums add, extremes only move outward."""
    return (seed[0] + table[0], seed[1] + table[1], np.minimum(seed[2], table[2]), np.maximum(seed[3], table[3]))


def labelings(n, rows):
    """One group (whole waves of one group: the reduction); two alternating groups (split lanes); a group held only by queries;
    labels -1 on a query, on old genomes and beside a diagonal."""
    g = np.arange(n, dtype=np.int32)
    out = {"one": (np.zeros(n, dtype=np.int32), 1), "alternating": (g % 2, 2)}
    only = (g % 2).astype(np.int32)
    only[list(rows)] = 2
    out["queries_only"] = (only, 3)
    loose = ((g // 3) % 3).astype(np.int32)
    for x in {rows[0], rows[-1] - 1, n // 2, n // 3} & set(range(n)):
        if n > 3 or x == rows[0]:
            loose[x] = -1
    out["unlabelled"] = (loose, 3)
    return out


def query_rows(n, how_many):
    """Up to ``how_many`` query rows: the last genome first (its row's live elements all lie before the diagonal), then genome 1, the
    middle and genome 0."""
    order = list(dict.fromkeys(x for x in (n - 1, 1, n // 2, 0) if 0 <= x < n))
    return sorted(order[:how_many])


POOLS = {"distinct": None, "ties": (0, 1, 250000, 499999, 500001, MILLION), "ends": (0, MILLION)}


def inputs(n, all_rows=False):
    """The inputs of shape n: 1 .. 3 query rows (or all n), the four labellings, the three value sets."""
    out = []
    for i, how_many in enumerate((1, 2, 3) if not all_rows else (n,)):
        rows = list(range(n)) if all_rows else query_rows(n, min(how_many, n))
        for kind, (label, n_groups) in labelings(n, rows).items():
            for pool_tag, pool in POOLS.items():
                if all_rows and pool_tag == "distinct":
                    pool_tag, pool = "wide", tuple(range(0, MILLION + 1, 7))      # (n^2 values: not all distinct)
                out.append(Input(f"n{n}_r{len(rows)}_{kind}_{pool_tag}", n, label, n_groups, rows, 7000 * n + 100 * i + len(out), pool))
    return out


def many_groups_input(n=SEGMENT + 1, n_groups=2048):
    """2,048 round-robin groups on n = 4,097: the largest LDS table, two segments, every lane of a wave another group."""
    return Input(f"n{n}_G{n_groups}", n, np.arange(n, dtype=np.int32) % n_groups, n_groups, [0, n // 2, n - 1], 99)


def refused_inputs():
    """(tag, Input, slab, refused pairs): a LIVE 2.0 and a LIVE 0.1234565 (no millionth), in a query-old pair and in the live copy of a
    pair of two queries."""
    n = 130
    rows = [1, 64, 129]
    x = Input("refused", n, np.arange(n, dtype=np.int32) % 3, 3, rows, 4242)
    out = []
    for tag, bad in (("two", 2.0), ("no_millionth", 0.1234565)):
        for where, places in (("query_old", [(1, 40)]), ("query_query", [(0, 64)]), ("both", [(1, 40), (0, 64), (2, 0)])):
            slab = x.slab()
            for p in places:
                assert x.live()[p], (tag, p)
                slab[p] = bad
            out.append((f"{tag}_{where}", x, slab, len(places)))
    return out
