"""The host side of the rows-value tests (no GPU): the references of tests/rows_value_cases.py held to the host statements the project
already trusts (``SparseEdges`` / ``Components`` / ``SingleLinkageTree`` / ``NearestNeighbors`` ``.extended`` and ``.from_dense``), the
generators' own promises, the references' indifference to what the dead elements hold -- and, on every input that
tests/rows_values_driver.py runs, the proof that the poison bites: a reference that read the dead elements gives another answer.  Then
the rows hook's refusal in the release library (pc_hook_rows_values) and its acceptance in the twin.

If a reference and a trusted statement disagree here, the reference is wrong."""

import ctypes
import os
import re

import numpy as np
import pytest

import rows_value_cases as rc
import slab_value_cases as tri
from conftest import REPO

N = 40
NAMES = [f"g{k:03d}" for k in range(N)]
QUERY_SETS = {"first": [0], "last": [N - 1], "adjacent": [19, 20], "every second": list(range(0, N, 2)), "scattered": [3, 4, 17, 30, 39],
              "all but one": [g for g in range(N) if g != 13]}
GENERATORS = {"tie_set": lambda: tri.tie_set(N, 5), "spread": lambda: tri.spread(N, 6)}
POISONS = (0.0, 1.0, 0.5, float("nan"), float("inf"), float("-inf"), 0.123456)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def matrix_of(values, names, as_distance=True):
    from phamclust_amd.matrix import SymMatrix
    n = len(names)
    matrix = SymMatrix.from_condensed(names, tri.square(values, n)[np.triu_indices(n, k=1)], is_distance=as_distance)
    matrix.lock()
    return matrix


def blocks(values, rows, as_distance):
    """(old genomes, the old block's matrix, the whole matrix, the symmetric rows slab)."""
    old, old_triangle = rc.old_block(values, N, rows)
    return old, matrix_of(old_triangle, [NAMES[g] for g in old], as_distance), matrix_of(values, NAMES, as_distance), rc.rows_of(values, N, rows)


def same_arrays(got, want):
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)


# ---- the generators ------------------------------------------------------------------------------------------------
def test_live_elements_are_the_projects():
    from phamclust_amd.matrix import _live_row_pairs
    for rows in QUERY_SETS.values():
        slab = np.arange(len(rows) * N, dtype=np.float64).reshape(len(rows), N)        # every element its own value
        same_arrays(rc.pairs_read(rows, slab, N), _live_row_pairs(N, np.asarray(rows, dtype=np.int64), slab))
        live, dead, diagonal = rc.live_mask(rows, N), rc.dead_mask(rows, N), rc.diagonal_mask(rows, N)
        assert not (dead & diagonal).any() and (live ^ (dead | diagonal)).all()
        assert diagonal.sum() == len(rows) and dead.sum() == len(rows) * (len(rows) - 1) // 2
        assert live.sum() == len(rows) * (N - 1) - len(rows) * (len(rows) - 1) // 2      # every pair that touches a query genome, once
        s, t, _ = rc.pairs_read(rows, slab, N, read="all")
        assert s.shape[0] == len(rows) * N and (s == t).sum() == len(rows)


def test_generators_keep_their_promises():
    for name, rows in QUERY_SETS.items():
        values = tri.spread(N, 3)
        slab = rc.rows_of(values, N, rows)
        full = tri.square(values, N)
        assert slab.shape == (len(rows), N) and slab.flags.c_contiguous and np.array_equal(slab, full[rows])
        marked = rc.poisoned(slab, rows, N, -7.0, -9.0)
        assert np.array_equal(np.argwhere(marked == -7.0), [[k, q] for k, q in enumerate(rows)])
        assert np.array_equal(marked == -9.0, rc.dead_mask(rows, N)) and np.array_equal(marked[rc.live_mask(rows, N)], slab[rc.live_mask(rows, N)])
        assert np.array_equal(rc.poisoned(slab, rows, N, -7.0) == -7.0, rc.diagonal_mask(rows, N)) and np.array_equal(slab, full[rows])
        query = rc.query_mask(rows, N)
        old = np.flatnonzero(~query)
        labels = rc.labelling_seed(N, rows, 4)
        assert labels.dtype == np.int32 and (labels[labels] == labels).all() and (labels <= np.arange(N)).all() and (labels[query] == np.flatnonzero(query)).all()
        assert all(labels[g] == np.flatnonzero(labels == labels[g]).min() for g in range(N))
        src, tgt, val = rc.forest_seed(N, rows, 4, micros=tri.TIE_MICROS)
        assert (src < tgt).all() and not query[src].any() and not query[tgt].any() and set(tri.micros_of(val).tolist()) <= set(tri.TIE_MICROS)
        forest = tri._UnionFind(N)
        assert all(forest.union(a, b) for a, b in zip(src.tolist(), tgt.tolist()))       # no cycle: a forest
        if old.shape[0] > 3:
            assert 0 < src.shape[0] <= old.shape[0] - 1
        for as_distance in (True, False):
            k_seed = max(min(5, old.shape[0] - 1), 0)
            nbr, val = rc.lists_seed(N, rows, k_seed, 4, as_distance)
            assert nbr.shape == val.shape == (N, k_seed) and (nbr[query] == -7).all() and np.isnan(val[query]).all()
            for g in old.tolist():
                assert not query[nbr[g]].any() and (nbr[g] != g).all() and np.unique(nbr[g]).shape[0] == k_seed and np.isfinite(val[g]).all()
                key = rc.order_key(val[g], as_distance)
                assert all(key[j] < key[j + 1] or (key[j] == key[j + 1] and nbr[g, j] < nbr[g, j + 1]) for j in range(k_seed - 1))
    pool = rc.finite_pool(1)
    assert (bits(pool) == bits(-0.0)).any() and (bits(pool) == bits(0.0)).any() and np.isfinite(pool).all()


def test_united_is_union_find():
    rng = np.random.default_rng(8)
    for pairs in (0, 5, 30, 200):
        s, t = rng.integers(0, N, size=pairs), rng.integers(0, N, size=pairs)
        start = rc.labelling_seed(N, [0, 7], 9)
        forest = tri._UnionFind(N)
        for g in range(N):
            forest.union(g, int(start[g]))
        for a, b in zip(s.tolist(), t.tolist()):
            forest.union(a, b)
        assert np.array_equal(rc.united(start, s, t), forest.labels())


# ---- the references against the trusted statements ------------------------------------------------------------------------
@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_edges_and_components_are_the_extended_statements(name, as_distance):
    from phamclust_amd.matrix import Components, SparseEdges
    values = GENERATORS[name]()
    present = np.unique(values)
    best = rc.best_value(as_distance)
    for rows in QUERY_SETS.values():
        old, old_matrix, whole, slab = blocks(values, rows, as_distance)
        marked = rc.poisoned(slab, rows, N, best, best)
        for threshold in [0.0, 1.0, 0.25] + present[:: max(1, present.shape[0] // 4)].tolist():
            stored = SparseEdges.from_dense(old_matrix, threshold)
            grown = stored.extended(NAMES, rows, slab)
            stated = SparseEdges.from_dense(whole, threshold)
            mine = rc.edges(rows, marked, N, threshold, as_distance)
            merged = rc.merged_edges((stored.source, stored.target, stored.weight), old, mine)
            same_arrays(merged, (grown.source, grown.target, grown.weight))
            same_arrays(merged, (stated.source, stated.target, stated.weight))
            touches = rc.query_mask(rows, N)[grown.source] | rc.query_mask(rows, N)[grown.target]
            same_arrays(mine, (grown.source[touches], grown.target[touches], grown.weight[touches]))
            every_old = SparseEdges.from_dense(old_matrix, 1.0 if as_distance else 0.0)
            every = SparseEdges.from_dense(whole, 1.0 if as_distance else 0.0)
            for strict in (True, False):
                stored_labels = Components(old_matrix.nodes, every_old.components(threshold, strict=strict))
                seed = np.arange(N, dtype=np.int32)
                seed[old] = old[stored_labels.labels]
                labels, n_pass = rc.components(seed, rows, marked, N, threshold, as_distance, strict)
                assert np.array_equal(labels, stored_labels.extended(NAMES, rows, slab, threshold, is_distance=as_distance, strict=strict).labels)
                assert np.array_equal(labels, every.components(threshold, strict=strict))
                whole_count = tri.components(values, N, threshold, as_distance, strict)[1]
                assert n_pass == whole_count - tri.components(rc.old_block(values, N, rows)[1], old.shape[0], threshold, as_distance, strict)[1]
            assert rc.components(None, rows, marked, N, threshold, as_distance, False)[1] == mine[0].shape[0]


@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_tree_is_the_extended_statement(name, as_distance):
    from phamclust_amd.matrix import SingleLinkageTree
    values = GENERATORS[name]()
    for rows in QUERY_SETS.values():
        old, old_matrix, whole, slab = blocks(values, rows, as_distance)
        stored = SingleLinkageTree.from_dense(old_matrix)
        seed = (old[stored.source], old[stored.target], stored.weight)
        mine = rc.tree(seed, rows, rc.poisoned(slab, rows, N, rc.NAN, rc.NAN), N, as_distance)
        grown, stated = stored.extended(NAMES, rows, slab), SingleLinkageTree.from_dense(whole)
        same_arrays(mine, (grown.source, grown.target, grown.weight))
        same_arrays(mine, (stated.source, stated.target, stated.weight))
        same_arrays(mine, tri.kruskal(values, N, as_distance))


@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_nearest_is_the_extended_statement(name, as_distance):
    from phamclust_amd.matrix import NearestNeighbors
    values = GENERATORS[name]()
    for rows in QUERY_SETS.values():
        old, old_matrix, whole, slab = blocks(values, rows, as_distance)
        marked = rc.poisoned(slab, rows, N, rc.best_value(as_distance))
        for k in (1, 7, N - 1, 64):
            stored = NearestNeighbors.from_dense(old_matrix, k)
            seed = None
            if old.shape[0] > 1:
                nbr, val = np.full((N, stored.k), -7, dtype=np.int32), np.full((N, stored.k), np.nan)
                nbr[old], val[old] = old[stored.indices], stored.weights
                seed = (nbr, val)
            mine = rc.nearest(seed, rows, marked, N, k, as_distance)
            grown, stated = stored.extended(NAMES, rows, slab, k), NearestNeighbors.from_dense(whole, k)
            same_arrays(mine, (grown.indices, bits(grown.weights)))
            same_arrays(mine, (stated.indices, bits(stated.weights)))
            same_arrays(mine, tri.nearest(values, N, k, as_distance))


def test_nearest_cuts_a_seed_that_is_longer_than_needed():
    """Columns of a seed beyond kk are cut, and a contract-only seed longer than needed gives what its first kk columns give."""
    rows = QUERY_SETS["scattered"]
    slab = rc.poisoned(rc.rows_of(tri.tie_set(N, 5), N, rows), rows, N, -np.inf)
    nbr, val = rc.lists_seed(N, rows, 9, 3, pool=tri.of_micros(tri.TIE_MICROS))
    same_arrays(rc.nearest((nbr, val), rows, slab, N, 6), rc.nearest((nbr[:, :6].copy(), val[:, :6].copy()), rows, slab, N, 6))
    assert rc.seed_k(N, 5, 6, False) == 6 and rc.seed_k(N, 5, 6, True) == 9 and rc.seed_k(N, 38, 6, False) == 1 == rc.seed_k(N, 38, 6, True)


# ---- the poison ----------------------------------------------------------------------------------------------------
def test_references_do_not_read_the_dead_elements():
    values = tri.tie_set(N, 5)
    for rows in QUERY_SETS.values():
        base = rc.rows_of(values, N, rows)
        labels, forest = rc.labelling_seed(N, rows, 2), rc.forest_seed(N, rows, 2, micros=tri.TIE_MICROS)
        k_seed = rc.seed_k(N, len(rows), 7, False)
        lists = rc.lists_seed(N, rows, k_seed, 2, pool=tri.of_micros(tri.TIE_MICROS)) if N - len(rows) > 1 else None
        want = None
        for poison in POISONS:
            marked = rc.poisoned(base, rows, N, poison, poison)
            got = (rc.edges(rows, marked, N, 0.5), rc.components(labels, rows, marked, N, 0.5)[:1], (rc.components(labels, rows, marked, N, 0.5)[1],),
                   rc.tree(forest, rows, marked, N), rc.nearest(lists, rows, rc.poisoned(base, rows, N, poison), N, 7))
            want = want or got
            for a, b in zip(got, want):
                same_arrays(a, b)


def bites_flat(x):
    """How a flat pass that read a dead element of the input would show: a longer edge list, a larger count, a refused tree."""
    threshold = x.thresholds[-1]
    live, dead = (rc.edges(x.rows, x.slab, x.n, threshold, x.as_distance, read) for read in ("live", "all"))
    assert live[0].shape[0] < dead[0].shape[0], x.label
    for strict in (True, False):
        live, dead = (rc.components(x.labels, x.rows, x.slab, x.n, threshold, x.as_distance, strict, read) for read in ("live", "all"))
        assert live[1] < dead[1], x.label                                    # (the labels need not differ; the count the fill returns does)
    if x.tree_slab is not None:
        assert len(rc.tree(x.forest, x.rows, x.tree_slab, x.n, x.as_distance)[0]) == x.n - 1
        with pytest.raises(rc.Refused):
            rc.tree(x.forest, x.rows, x.tree_slab, x.n, x.as_distance, read="all")


@pytest.mark.parametrize("n", rc.FLAT_SHAPES)
def test_the_poison_bites_on_the_flat_inputs(n):
    count = 0
    for x in rc.flat_inputs(n):
        bites_flat(x)
        count += 1
    assert count == (6 if n <= 65 else 5) * 4 * 2


def test_the_poison_bites_on_the_tiny_and_the_wide_inputs():
    for x in list(rc.tiny_inputs()) + list(rc.wide_inputs()):
        bites_flat(x)
    n, rows = rc.WIDE_SHAPE
    assert len(rows) * n >= 3 * rc.CHUNK > (len(rows) - 1) * n and n > rc.CHUNK


@pytest.mark.parametrize("n", [2, 3, 64, 65, 129, 130])
def test_the_poison_bites_on_the_nearest_inputs(n):
    """A diagonal taken for a candidate lands first in that genome's list: the genome names itself."""
    seen = set()
    for x in rc.nearest_inputs(n):
        live, dead = (rc.nearest(x.seed, x.rows, x.slab, x.n, x.k, x.as_distance, read) for read in ("live", "all"))
        assert (live[0] != np.arange(n)[:, None]).all() and (dead[0][x.rows, 0] == x.rows).all(), x.label
        seen.add((x.rows.shape[0], x.k))
    assert {m for m, _ in seen} >= ({1, n} | ({63, 64, 65} if n >= 129 else {63} if n >= 64 else set()))
    assert {k for _, k in seen} == set(rc.nearest_ks(n))


def test_nearest_inputs_hold_the_hard_seeds():
    """Among the inputs: a seed list with -0.0 and +0.0 side by side, and a new candidate that ties a stored entry's value with a smaller
    and with a larger index."""
    zeros_side_by_side = ties_smaller = ties_larger = 0
    for x in rc.nearest_inputs(129):
        if x.seed is None:
            continue
        nbr, val = x.seed
        old = np.flatnonzero(~rc.query_mask(x.rows, x.n))
        if x.label[2] == "finite" and val.shape[1] > 1:
            b = bits(val[old])
            zeros_side_by_side += int((((b[:, :-1] == bits(-0.0)) & (b[:, 1:] == bits(0.0))) | ((b[:, :-1] == bits(0.0)) & (b[:, 1:] == bits(-0.0)))).sum())
        if x.label[2] == "tie_set":
            for k, q in enumerate(x.rows.tolist()):
                tie = bits(val[old]) == bits(x.slab[k, old])[:, None]
                ties_smaller += int((tie & (nbr[old] < q)).sum())
                ties_larger += int((tie & (nbr[old] > q)).sum())
    assert zeros_side_by_side > 100 and ties_smaller > 100 and ties_larger > 100


# ---- the library's new entry point -----------------------------------------------------------------------------------
def twins():
    from phamclust_amd import hip
    return [hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")]


def test_the_rows_hook_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    assert re.search(r"\bint pc_hook_rows_values\s*\(const double\* values, int32_t n_rows, int32_t n\)", header)
    assert "pc_hook_rows_values" in hip.EXPORTS and hip.EXPORTS.count("pc_hook_rows_values") == 1
    for lib in twins():
        assert hasattr(ctypes.CDLL(lib), "pc_hook_rows_values"), lib
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 167 and hip.load().pc_version() >= 167
    table = header.split("only in libphamclust_hip_hooks.so")[1]
    assert "pc_hook_rows_values" in table and "pc_hook_slab_values" in table
    for doc in ("INTEGRATION.md", os.path.join("docs", "history.md")):
        assert "pc_hook_rows_values" in open(os.path.join(REPO, doc)).read(), doc
    assert callable(hip.set_rows_values) and callable(hip.set_slab_values)


def test_the_release_library_refuses_rows_values(native_built):
    from phamclust_amd import hip
    assert hip.load().pc_test_hooks() == 0
    lib = ctypes.CDLL(hip.LIB_PATH)
    lib.pc_hook_rows_values.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int32]
    lib.pc_last_error.restype = ctypes.c_char_p
    values = np.zeros((2, 5))
    assert lib.pc_hook_rows_values(values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 2, 5) == -3
    assert lib.pc_last_error() == b"pc_hook_rows_values: this library carries no test hooks (libphamclust_hip_hooks.so does)"      # its sibling's wording
    assert lib.pc_hook_rows_values(None, 0, 0) == -3
    with pytest.raises(hip.HipLibraryError, match="status -3"):
        hip.set_rows_values(values)
    with pytest.raises(hip.HipLibraryError, match="status -3"):
        hip.set_rows_values(None)
    assert hip._rows_values is None and hip._slab_values is None              # nothing kept
    for wrong in (values.astype(np.float32), np.zeros(10), np.zeros((2, 10))[:, ::2], [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="float64"):
            hip.set_rows_values(wrong)


def test_the_hooks_twin_takes_rows_values(native_built):
    lib = ctypes.CDLL(twins()[1])
    lib.pc_hook_rows_values.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int32]
    values = np.zeros((2, 5))
    pointer = values.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.pc_test_hooks() == 1
    assert lib.pc_hook_rows_values(pointer, 2, 5) == 0 and lib.pc_hook_rows_values(pointer, -1, 5) == -1 and lib.pc_hook_rows_values(pointer, 2, -5) == -1
    assert lib.pc_hook_rows_values(None, 0, 0) == 0 and lib.pc_hook_rows_values(None, 3, 4) == 0
