"""The host side of the slab-value tests (no GPU): the references of tests/slab_value_cases.py held to the host statements the project
already trusts, the generators' own promises, the range cut of the affinity fill's column pass as host arithmetic
(pc_affinity_ranges), and the value hook's refusal in the release library (pc_hook_slab_values).

If a reference and a trusted statement disagree here, the reference is wrong."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

import slab_value_cases as cases
from conftest import REPO

N = 40
NEW_EXPORTS = ("pc_hook_slab_values", "pc_affinity_ranges")
GENERATORS = {"tie_set": lambda: cases.tie_set(N, 5), "spread": lambda: cases.spread(N, 6)}
NAMES = [f"g{k:03d}" for k in range(N)]


def matrix_of(values, as_distance=True):
    """The SymMatrix whose weights are the triangle's (a similarity matrix: the values taken as similarities)."""
    from phamclust_amd.matrix import SymMatrix
    full = cases.square(values, N)
    matrix = SymMatrix.from_condensed(NAMES, full[np.triu_indices(N, k=1)], is_distance=as_distance)
    matrix.lock()
    return matrix


def labelings():
    rng = np.random.default_rng(9)
    return {"mod 5": (np.arange(N) % 5, 5), "blocks": (np.arange(N) // 16, 3), "singletons": (np.arange(N), N),
            "with empty groups": (rng.choice([0, 2, 3, 6], size=N), 8)}


def groups_of(group, n_groups):
    return [[NAMES[g] for g in range(N) if group[g] == a] for a in range(n_groups)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the generators ------------------------------------------------------------------------------------------------
def test_generators_keep_their_promises():
    for n in (2, 3, 40, 130):
        for values in (cases.two_valued(n, 0.5, 1), cases.tie_set(n, 2), cases.spread(n, 3), cases.ramp(n), cases.finite_doubles(n, 4)):
            assert values.dtype == np.float64 and values.shape == (cases.n_pairs(n),) and values.flags.c_contiguous
            assert np.isfinite(values).all()
    assert set(np.unique(cases.two_valued(130, 0.5, 1)).tolist()) == {0.0, 1e-6}
    assert abs((cases.two_valued(130, 0.02, 1) == 0.0).mean() - 0.02) < 0.01
    assert set(cases.micros_of(cases.rescaled(cases.two_valued(40, 0.5, 1), 499999, 500000)).tolist()) == {499999, 500000}
    assert set(cases.micros_of(cases.tie_set(130, 2)).tolist()) == set(cases.TIE_MICROS)
    assert np.array_equal(cases.tie_set(130, 2), cases.tie_set(130, 2)) and not np.array_equal(cases.tie_set(130, 2), cases.tie_set(130, 3))
    micro = cases.micros_of(cases.spread(515, 3))
    assert micro.min() < 100 and micro.max() > MILLION - 100
    # ramp: every element of a triangle up to 1,414 genomes differs from every other; beyond, every row's elements and the elements above them
    ramp = cases.micros_of(cases.ramp(515))
    assert np.unique(ramp).shape[0] == ramp.shape[0]
    assert math.gcd(cases.RAMP_STRIDE, MILLION) == 1 and math.gcd(cases.RAMP_STRIDE, MILLION + 1) == 1
    big = cases.micros_of(cases.ramp(4099))
    row = big[cases.pair_index(0, 4098):]
    assert row.shape[0] == 4098 and np.unique(row).shape[0] == 4098 and (row != big[cases.pair_index(0, 4097):cases.pair_index(0, 4098)][:1]).all()
    # finite doubles: what the pool promises
    wild = cases.finite_doubles(130, 4)
    key = cases.total_order_key(wild)
    assert (wild < 0).any() and (wild > 1).any() and (bits(wild) == bits(-0.0)).any() and (bits(wild) == bits(0.0)).any()
    assert ((wild != 0) & (np.abs(wild) < 2.2250738585072014e-308)).any()
    gaps = np.diff(np.unique(key))
    assert (gaps == 1).sum() >= 10                                           # neighbours in the total order: one ulp apart (and the two zeros)
    order = np.argsort(key, kind="stable")
    assert (np.diff(wild[order]) >= 0).all() and key[bits(wild) == bits(-0.0)][0] + 1 == key[bits(wild) == bits(0.0)][0]


MILLION = cases.MILLION


def test_with_bad_values_are_what_the_checks_refuse():
    values = cases.spread(N, 6)
    at = [0, 5, 17, 100, 333, cases.n_pairs(N) - 1, 400]
    bad = cases.with_bad(values, at)
    assert np.array_equal(np.flatnonzero(bits(bad) != bits(values)), sorted(at)) and np.array_equal(values, cases.spread(N, 6))
    k = np.rint(bad[at] * 1.0e6)
    with np.errstate(invalid="ignore"):
        refused = ~((k >= 0.0) & (k <= 1.0e6)) | (k / 1000000.0 != bad[at])
    assert refused.all()
    zero = np.array([-0.0])
    k = np.rint(zero * 1.0e6)
    assert (k >= 0.0).all() and (k / 1000000.0 == zero).all() and cases.micros_of(zero)[0] == 0       # -0.0 is a valid zero


# ---- the references against the trusted statements ------------------------------------------------------------------------
@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_kruskal_is_single_linkage_tree_from_dense(name, as_distance):
    from phamclust_amd.matrix import SingleLinkageTree
    values = GENERATORS[name]()
    tree = SingleLinkageTree.from_dense(matrix_of(values, as_distance))
    src, tgt, val = cases.kruskal(values, N, as_distance)
    assert np.array_equal(src, tree.source) and np.array_equal(tgt, tree.target) and np.array_equal(bits(val), bits(tree.weight))


@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_edges_and_components_are_sparse_edges_from_dense(name, as_distance):
    from phamclust_amd.matrix import SparseEdges
    values = GENERATORS[name]()
    matrix = matrix_of(values, as_distance)
    present = np.unique(values)
    for threshold in [0.0, 1.0, 0.25] + present[:: max(1, present.shape[0] // 6)].tolist():
        edges = SparseEdges.from_dense(matrix, threshold)
        src, tgt, val = cases.edge_list(values, N, threshold, as_distance, strict=False)
        assert np.array_equal(src, edges.source) and np.array_equal(tgt, edges.target) and np.array_equal(bits(val), bits(edges.weight))
        whole = SparseEdges.from_dense(matrix, 1.0 if as_distance else 0.0)
        for strict in (True, False):
            labels, n_pass = cases.components(values, N, threshold, as_distance, strict)
            assert np.array_equal(labels, whole.components(threshold, strict=strict)), (threshold, strict)
            assert n_pass == cases.edge_list(values, N, threshold, as_distance, strict)[0].shape[0]
        assert cases.components(values, N, threshold, as_distance, False)[1] == len(edges)


@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_nearest_is_nearest_neighbors_from_dense(name, as_distance):
    from phamclust_amd.matrix import NearestNeighbors
    values = GENERATORS[name]()
    matrix = matrix_of(values, as_distance)
    for k in (1, 7, N - 1, 64):
        want = NearestNeighbors.from_dense(matrix, k)
        nbr, val = cases.nearest(values, N, k, as_distance)
        assert nbr.shape == want.indices.shape == (N, min(k, N - 1))
        assert np.array_equal(nbr, want.indices) and np.array_equal(val, bits(want.weights))


def test_nearest_on_finite_doubles_orders_the_zeros():
    """Where the trusted statement (a plain float compare) has no opinion: -0.0 comes before +0.0, then the index."""
    values = np.array([0.0, -0.0, -0.0, 5e-324, -5e-324, 0.0])                # pairs (0,1) (0,2) (1,2) (0,3) (1,3) (2,3)
    nbr, val = cases.nearest(values, 4, 3, True)
    assert nbr[0].tolist() == [2, 1, 3] and val[0].tolist() == bits([-0.0, 0.0, 5e-324]).tolist()
    assert nbr[3].tolist() == [1, 2, 0]
    nbr, val = cases.nearest(values, 4, 3, False)
    assert nbr[0].tolist() == [3, 1, 2] and nbr[3].tolist() == [0, 2, 1]


@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_between_is_group_linkage_from_dense(name, as_distance):
    from phamclust_amd.matrix import GroupLinkage
    values = GENERATORS[name]()
    matrix = matrix_of(values)
    for label, (group, n_groups) in labelings().items():
        want = GroupLinkage.from_dense(matrix, groups_of(group, n_groups))
        if not as_distance:
            want = want.inverted()
        total, count, lo, hi = cases.between(values, N, group, n_groups, as_distance)
        for got, stated in ((total, want.sum), (count, want.cnt), (lo, want.lo), (hi, want.hi)):
            assert got.dtype == stated.dtype and np.array_equal(got, stated), label


@pytest.mark.parametrize("as_distance", [True, False])
@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_affinity_is_group_affinity_from_dense(name, as_distance):
    from phamclust_amd.matrix import GroupAffinity
    values = GENERATORS[name]()
    matrix = matrix_of(values)
    for label, (group, n_groups) in labelings().items():
        want = GroupAffinity.from_dense(matrix, groups_of(group, n_groups))
        if not as_distance:
            want = want.inverted()
        got = cases.affinity(values, N, group, n_groups, as_distance)
        for key in ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi"):
            assert got[key].dtype == getattr(want, key).dtype and np.array_equal(got[key], getattr(want, key)), (label, key)
        for a, b in zip(got["table"], want.table):
            assert a.dtype == b.dtype and np.array_equal(a, b), label


def test_affinity_mean_tie_goes_to_the_smaller_group():
    """Groups of sizes 2 and 3 whose sums to genome 0 are 2 : 3 -- equal means -- and a group of larger mean in front of both."""
    n, group = 7, np.array([3, 2, 2, 1, 1, 1, 0])
    full = np.zeros((n, n), dtype=np.int64)
    full[0, 1], full[0, 2] = 300000, 100000                                  # group 2: sum 400,000 over 2
    full[0, 3], full[0, 4], full[0, 5] = 100000, 200000, 300000              # group 1: sum 600,000 over 3
    full[0, 6] = 900000                                                      # group 0: the larger mean
    full = full + full.T
    got = cases.affinity(cases.of_micros(full[np.tril_indices(n, k=-1)]), n, group, 4)
    assert got["near_group"][0, 0] == 1 and got["near_sum"][0] == 600000
    assert got["near_group"][1, 0] == 1 and got["near_group"][2, 0] == 1      # by minimum 100,000 twice, by maximum 300,000 twice: the smaller index
    swapped = np.array([3, 1, 1, 2, 2, 2, 0])                                # the same two groups under the other two indices
    got = cases.affinity(cases.of_micros(full[np.tril_indices(n, k=-1)]), n, swapped, 4)
    assert got["near_group"][:, 0].tolist() == [1, 1, 1] and got["near_sum"][0] == 400000


# ---- the library's two new entry points -----------------------------------------------------------------------------------
def twins():
    from phamclust_amd import hip
    return [hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")]


def test_new_entry_points_are_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in twins():
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 166 and hip.load().pc_version() >= 166
    assert "pc_hook_slab_values" in header.split("only in libphamclust_hip_hooks.so")[1]
    for doc in ("INTEGRATION.md", os.path.join("docs", "history.md")):
        text = open(os.path.join(REPO, doc)).read()
        assert all(name in text for name in NEW_EXPORTS), doc


def test_the_release_library_refuses_slab_values(native_built):
    from phamclust_amd import hip
    assert hip.load().pc_test_hooks() == 0
    lib = ctypes.CDLL(hip.LIB_PATH)
    lib.pc_hook_slab_values.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int64]
    lib.pc_last_error.restype = ctypes.c_char_p
    values = cases.spread(4, 1)
    assert lib.pc_hook_slab_values(values.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), values.shape[0]) == -3
    assert b"pc_hook_slab_values" in lib.pc_last_error() and b"hooks" in lib.pc_last_error()
    assert lib.pc_hook_slab_values(None, 0) == -3
    with pytest.raises(hip.HipLibraryError, match="status -3"):
        hip.set_slab_values(values)
    with pytest.raises(hip.HipLibraryError, match="status -3"):
        hip.set_slab_values(None)
    assert hip._slab_values is None                                          # nothing kept
    for wrong in (values.astype(np.float32), np.zeros((2, 3)), np.zeros(12)[::2], [0.0, 1.0]):
        with pytest.raises(ValueError, match="float64"):
            hip.set_slab_values(wrong)


def test_the_hooks_twin_takes_slab_values(native_built):
    lib = ctypes.CDLL(twins()[1])
    lib.pc_hook_slab_values.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int64]
    values = cases.spread(4, 1)
    pointer = values.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.pc_test_hooks() == 1
    assert lib.pc_hook_slab_values(pointer, values.shape[0]) == 0 and lib.pc_hook_slab_values(pointer, -1) == -1
    assert lib.pc_hook_slab_values(None, 0) == 0 and lib.pc_hook_slab_values(None, 5) == 0


def test_triangle_helpers_round_trip():
    from phamclust_amd import hip
    for n in (0, 1, 2, 3, 40):
        values = cases.spread(n, n)
        full = hip.square_of(values, n)
        assert full.shape == (n, n) and np.array_equal(full, full.T) and np.array_equal(full, cases.square(values, n))
        assert np.array_equal(hip.triangle_of(full), values)
        assert all(full[s, t] == values[cases.pair_index(s, t)] for t in range(n) for s in range(t))
    assert (np.diag(hip.square_of(cases.spread(5, 1), 5, diagonal=1.0)) == 1.0).all()
    with pytest.raises(ValueError):
        hip.square_of(np.zeros(5), 4)
    with pytest.raises(ValueError):
        hip.triangle_of(np.zeros((3, 4)))


def range_cases():
    """(goff, G, N) of random labelings: empty groups, one giant group, G from 1 to 2,048."""
    rng = np.random.default_rng(17)
    out = []
    for n_groups in (1, 2, 3, 5, 63, 64, 65, 600, 2047, 2048):
        for n in (1, 65, 2049, 20000):
            sizes = np.bincount(rng.integers(0, n_groups, size=n), minlength=n_groups)
            out.append(sizes)                                               # about equal, some empty when G is near or above N
            giant = np.zeros(n_groups, dtype=np.int64)
            giant[rng.integers(0, n_groups)] = max(n - min(n, n_groups) // 2, 1)
            rest = n - int(giant.sum())
            if rest > 0:
                giant += np.bincount(rng.integers(0, n_groups, size=rest), minlength=n_groups)
            out.append(giant)                                               # one group holds nearly everything
            sparse = np.zeros(n_groups, dtype=np.int64)
            some = rng.choice(n_groups, size=max(1, n_groups // 7), replace=False)
            sparse[some] = np.bincount(rng.integers(0, some.shape[0], size=n), minlength=some.shape[0])
            out.append(sparse)                                              # six groups in seven empty
    return [(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), int(sizes.shape[0]), int(sizes.sum())) for sizes in out]


def test_affinity_ranges_on_both_twins(native_built):
    pointer = ctypes.POINTER(ctypes.c_int32)
    checked = 0
    for path in twins():
        lib = ctypes.CDLL(path)
        lib.pc_affinity_ranges.argtypes = [pointer, ctypes.c_int, ctypes.c_int, ctypes.c_int, pointer, ctypes.c_int]
        for goff, n_groups, n in range_cases():
            for want in (-3, 0, 1, 2, 7, 64, 249, n_groups - 1, n_groups, n_groups + 1, 5000):
                bounds = np.full(n_groups + 2, -7, dtype=np.int32)
                r = lib.pc_affinity_ranges(goff.ctypes.data_as(pointer), n_groups, n, want, bounds.ctypes.data_as(pointer), bounds.shape[0])
                assert 1 <= r <= max(1, min(n_groups, want)), (n_groups, n, want, r)
                cut = bounds[:r + 1]
                assert cut[0] == 0 and cut[-1] == n_groups and (np.diff(cut) > 0).all(), (n_groups, n, want, cut)      # strictly ascending: no empty range
                assert bounds[r + 1] == -7
                assert lib.pc_affinity_ranges(goff.ctypes.data_as(pointer), n_groups, n, want, None, 0) == r          # the count alone
                checked += 1
        one = np.array([0, 4], dtype=np.int32)
        bounds = np.zeros(2, dtype=np.int32)
        assert lib.pc_affinity_ranges(None, 1, 4, 1, bounds.ctypes.data_as(pointer), 2) == -1
        assert lib.pc_affinity_ranges(one.ctypes.data_as(pointer), 1, 5, 1, bounds.ctypes.data_as(pointer), 2) == -1     # goff does not end at N
        assert lib.pc_affinity_ranges(one.ctypes.data_as(pointer), 1, 4, 1, bounds.ctypes.data_as(pointer), 1) == -1     # no room
        assert lib.pc_affinity_ranges(one.ctypes.data_as(pointer), 0, 4, 1, bounds.ctypes.data_as(pointer), 2) == -1
    assert checked > 2000


def test_affinity_ranges_balance_members(native_built):
    """What the cut is for: with groups of about equal size every range holds about N / R members, and the binding agrees."""
    from phamclust_amd.hip import Context
    n, n_groups = 2049, 600
    group = np.arange(n) % n_groups
    goff = cases.affinity_goff(group, n_groups)
    want = math.ceil(16 * 512 / math.ceil(n / Context.affinity_block()))
    cut = Context.affinity_ranges(goff, n, want)
    assert cut.shape[0] - 1 == want == 249 and (np.diff(cut) >= 2).all()      # every range: at least two non-empty groups
    members = np.diff(goff[cut])
    assert members.min() >= n // want - 4 and members.max() <= n // want + 8
    for fewer in (1, 2, 100):
        assert (np.diff(Context.affinity_ranges(goff, n, fewer)) >= 2).all()
    with pytest.raises(ValueError):
        Context.affinity_ranges([0, 3, 2], 2, 1)
