"""The edge, component and nearest fills over several GPUs from one process (pc_multi_fill_edges / _components / _nearest,
``MultiContext.fill_edges`` / ``fill_components`` / ``fill_nearest``, and ``--adjacency-only`` / ``--components-only`` / ``--nearest``
with ``--gpus N``), rehearsed as the other multi-GPU tests are: several contexts on device 0 in ONE process.

Every expectation is the single-context call's result on the same upload -- which tests/test_gpu_edges.py, test_gpu_components.py
and test_gpu_nearest.py hold to the reference's fixtures -- or, in one parametrisation per call, a dense golden file through the host
statements of the definitions (``SparseEdges.from_dense``, its ``components``, ``NearestNeighbors.from_dense``).  Every comparison is
``np.array_equal``: the result does not depend on the number of devices.  A merge that lets a sentinel displace an entry, loses a
tie between two devices' lists, misses the join of a component across a stretch boundary, lays the edge lists end to end in the
wrong order, or a call that leaves a context sharded fails here."""

import ctypes
import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, golden_file, read_lower_triangle, synth200_file
from test_gpu_components import hand_built as cc_hand_built
from test_gpu_edges import thresholds
from test_gpu_nearest import hand_built as nn_hand_built

pytestmark = pytest.mark.gpu

WORLDS = (2, 3, 5)


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


@pytest.fixture(scope="module")
def multis(native_built):
    """MultiContext([0] * world), made on first use and kept for the module (a context per device is the costly part)."""
    from phamclust_amd import hip
    made = {}

    def get(world):
        if world not in made:
            made[world] = hip.MultiContext([0] * world)
        return made[world]
    yield get
    for multi in made.values():
        multi.close()


def costs(ctx, packed, metric):
    """cost[t] of the deal as the header states it, recomputed on a single context: t for the set metrics, the COUNT walk's DP cells
    per target + 2000 t for aai / peq."""
    n = packed.n_genomes
    if metric not in ("aai", "peq", "aai_ppos"):
        return np.arange(n, dtype=np.uint64)
    ctx.set_shard(0, 1, balanced=True)                                     # (computes the target costs; one rank: every pair stays)
    cells = ctx.target_costs()
    ctx.set_shard(0, 1)
    return cells + np.arange(n, dtype=np.uint64) * np.uint64(2000)


def slabs_of(bounds, slab_bytes):
    """Slabs the devices cut together: the chunking rule over count[t] = t for the targets of each stretch."""
    from phamclust_amd.hip import Context
    return sum(len(Context.chunk_plan(np.arange(a, b, dtype=np.uint64), max(slab_bytes // 8, 1))) - 1 for a, b in zip(bounds, bounds[1:]) if b > a)


def check_route(st, world, bounds, n, slab_bytes, label):
    """The entries the route adds to the stats, the deal, and the slab count where the slab size is forced."""
    assert st["n_devices"] == world == len(st["per_device"]), label
    assert st["stretches"] == list(bounds), label
    assert st["n_pairs"] == n * (n - 1) // 2 == sum(p["n_pairs"] for p in st["per_device"]), label
    for r, per in enumerate(st["per_device"]):
        a, b = bounds[r], bounds[r + 1]
        assert per["n_pairs"] == b * (b - 1) // 2 - a * (a - 1) // 2, (label, r)
        if a == b:
            assert not any(per.values()), (label, r)                       # an empty stretch: zeros, nothing ran
    assert st["ms_exchange"] >= 0.0 and st["ms_merge"] >= 0.0 and len(st["peer_access"]["devices"]) == world, label
    if slab_bytes:
        assert st["n_slabs"] == slabs_of(bounds, slab_bytes), label


# ---- nearest ---------------------------------------------------------------------------------------------
NEAREST_SHAPES = [("identical", 130), ("valley", 129), ("chain", 65)]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("metric", ["jc", "peq"])
@pytest.mark.parametrize("kind,n", NEAREST_SHAPES)
def test_nearest_equals_the_single_context(ctx, multis, kind, n, metric, world):
    """identical: every value ties, so across devices the index alone decides who is listed; valley: insertions at every step from
    both passes; chain, N = 65 on five devices: stretch boundaries inside a block of 64 sources, and at k = 64 lists with sentinel
    tails (a device that holds few targets has met fewer than 64 candidates for most genomes)."""
    from phamclust_amd.hip import MultiContext
    packed = nn_hand_built(n, kind)
    ctx.upload(packed)
    multi = multis(world)
    multi.upload(packed, residues=False)                                   # the residues follow on demand, on every device
    bounds = MultiContext.slab_stretches(costs(ctx, packed, metric), world).tolist()
    assert bounds[0] == 0 and bounds[-1] == n and all(a < b for a, b in zip(bounds, bounds[1:]))
    if (n, world) == (65, 5):
        assert any(b % 64 for b in bounds[1:-1]) and bounds[-1] - bounds[-2] < 64      # the last device meets fewer than 64 targets
    for as_distance in (True, False):
        for k in (1, 63, 64):
            want_nbr, want_val = ctx.fill_nearest(metric, k, as_distance=as_distance)
            for slab_bytes in (0, 8 * 4000) + ((8,) if k != 63 else ()):
                label = (kind, n, metric, world, as_distance, k, slab_bytes)
                nbr, val, st = multi.fill_nearest(metric, k, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
                assert nbr.dtype == np.int32 and val.dtype == np.float64 and nbr.shape == val.shape == (n, k), label
                assert np.array_equal(nbr, want_nbr), label
                assert np.array_equal(val, want_val), label
                assert st["k"] == k, label
                check_route(st, world, bounds, n, slab_bytes, label)
                if kind == "identical":
                    assert nbr.tolist() == [[h for h in range(n) if h != g][:k] for g in range(n)], label


@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_fewer_genomes_than_devices(ctx, multis, metric):
    """One, two and three genomes on four devices: kk = min(k, N - 1), stretches that are empty, devices that launch nothing."""
    multi = multis(4)
    for n, bounds in ((1, [0, 1, 1, 1, 1]), (2, [0, 2, 2, 2, 2]), (3, None)):         # (no pair at all: the root serves the call alone)
        packed = nn_hand_built(n, "chain")
        ctx.upload(packed)
        multi.upload(packed)
        if bounds is None:
            from phamclust_amd.hip import MultiContext
            bounds = MultiContext.slab_stretches(costs(ctx, packed, metric), 4).tolist()
            assert bounds[:2] == [0, 2] and bounds[-2:] == [3, 3]          # at least one device without a target
        for as_distance in (True, False):
            for k in (1, 2, 5, 64):
                want_nbr, want_val, want_st = ctx.fill_nearest(metric, k, as_distance=as_distance, want_stats=True)
                for slab_bytes in (0, 8):
                    label = (n, metric, as_distance, k, slab_bytes)
                    nbr, val, st = multi.fill_nearest(metric, k, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
                    assert nbr.shape == val.shape == (n, min(k, n - 1)) and st["k"] == min(k, n - 1) == want_st["k"], label
                    assert np.array_equal(nbr, want_nbr) and np.array_equal(val, want_val), label
                    assert st["stretches"] == bounds and st["n_pairs"] == n * (n - 1) // 2, label
                    if n > 1:
                        check_route(st, 4, bounds, n, slab_bytes, label)
                    else:
                        assert st["n_slabs"] == 0 == want_st["n_slabs"], label
            labels, st = multi.fill_components(metric, 0.7, as_distance=as_distance, want_stats=True)
            want, want_st = ctx.fill_components(metric, 0.7, as_distance=as_distance, want_stats=True)
            assert np.array_equal(labels, want) and (st["n_components"], st["n_edges"]) == (want_st["n_components"], want_st["n_edges"])
            got = multi.fill_edges(metric, 0.7, as_distance=as_distance)
            for g, w in zip(got, ctx.fill_edges(metric, 0.7, as_distance=as_distance)):
                assert g.dtype == w.dtype and np.array_equal(g, w), (n, metric, as_distance)


# ---- components ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("metric", ["jc", "peq"])
@pytest.mark.parametrize("kind,n", [("chain", 300), ("disjoint", 70), ("identical", 70)])
def test_components_equal_the_single_context(ctx, multis, kind, n, metric, world):
    """chain: ONE component that crosses every stretch boundary -- each device holds a piece of the path and the merge must join
    at every boundary; disjoint: N roots; identical: every hook of every device aims at genome 0.  Thresholds at a value that
    occurs, strict and not, in both directions; the count of passing pairs summed over the devices is the single context's."""
    from phamclust_amd.hip import MultiContext
    packed = cc_hand_built(n, kind)
    ctx.upload(packed)
    multi = multis(world)
    multi.upload(packed, residues=False)
    bounds = MultiContext.slab_stretches(costs(ctx, packed, metric), world).tolist()
    forced = 8 * 300 if metric == "jc" else 8 * 3000                       # N = 300: ~250 slabs of a target or two; an aligned slab is a plan of its own: ~15
    for as_distance in (True, False):
        dense = np.asarray(ctx.fill(metric, as_distance=as_distance))
        s, t = np.triu_indices(n, k=1)
        value = float(dense[t - s == 1][0])                                # what neighbours are at: occurs in every collection
        beyond = 0.7 if as_distance else 0.3
        for thr in (value, beyond):
            for strict in (True, False):
                want, want_st = ctx.fill_components(metric, thr, as_distance=as_distance, strict=strict, want_stats=True)
                for slab_bytes in (0, forced):
                    label = (kind, n, metric, world, as_distance, thr, strict, slab_bytes)
                    labels, st = multi.fill_components(metric, thr, as_distance=as_distance, strict=strict, slab_bytes=slab_bytes, want_stats=True)
                    assert labels.dtype == np.int32 and labels.shape == (n,), label
                    assert np.array_equal(labels, want), label
                    assert st["n_components"] == want_st["n_components"] and st["n_edges"] == want_st["n_edges"], label
                    check_route(st, world, bounds, n, slab_bytes, label)
        if kind == "chain":                                                # the shapes are what they are meant to be
            labels, st = multi.fill_components(metric, value, as_distance=as_distance, strict=False, want_stats=True)
            assert not labels.any() and st["n_components"] == 1 and st["n_edges"] == n - 1
            labels, st = multi.fill_components(metric, value, as_distance=as_distance, strict=True, want_stats=True)
            assert np.array_equal(labels, np.arange(n)) and st["n_edges"] == 0
        elif kind == "disjoint":
            labels, st = multi.fill_components(metric, 0.999999 if as_distance else 0.000001, as_distance=as_distance, want_stats=True)
            assert np.array_equal(labels, np.arange(n)) and st["n_components"] == n and st["n_edges"] == 0
        else:
            labels, st = multi.fill_components(metric, value, as_distance=as_distance, strict=False, want_stats=True)
            assert not labels.any() and st["n_edges"] == n * (n - 1) // 2


# ---- edges -----------------------------------------------------------------------------------------------
def tail_built(n):
    """n genomes that share nothing, but for the last two, which are identical: the one pair that passes lies in the last stretch."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        for j in range(4):
            g.add(f"p{min(k, n - 2)}_{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        genomes.append(g)
    return pack_genomes(genomes)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("metric", ["jc", "peq"])
@pytest.mark.parametrize("kind,n", [("chain", 300), ("disjoint", 70), ("identical", 70), ("tail", 70)])
def test_edges_equal_the_single_context(ctx, multis, kind, n, metric, world):
    """The arrays equal the single context's element for element -- so they are sorted by (t, s) across the devices' lists -- at
    the thresholds of tests/test_gpu_edges.py, at one nothing passes, and (tail) at one only the last stretch contributes to."""
    from phamclust_amd.hip import MultiContext
    packed = tail_built(n) if kind == "tail" else cc_hand_built(n, kind)
    ctx.upload(packed)
    multi = multis(world)
    multi.upload(packed, residues=False)
    bounds = MultiContext.slab_stretches(costs(ctx, packed, metric), world).tolist()
    forced = 8 * 300 if metric == "jc" else 8 * 3000                       # (as for the components)
    for as_distance in (True, False):
        dense = np.asarray(ctx.fill(metric, as_distance=as_distance))
        if kind in ("chain", "tail"):
            some = thresholds(dense, as_distance)
        else:                                                              # one value everywhere: at it, and beside it
            some = [float(dense[0]), 0.75 if as_distance else 0.25]
        nothing = -1.0 if as_distance else 2.0
        for thr in some + [nothing]:
            want = ctx.fill_edges(metric, thr, as_distance=as_distance)
            for slab_bytes in (0, forced):
                label = (kind, n, metric, world, as_distance, thr, slab_bytes)
                *got, st = multi.fill_edges(metric, thr, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
                for name, g, w in zip(("src", "tgt", "val"), got, want):
                    assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.shape, w.shape)
                    assert np.array_equal(g, w), (label, name)
                assert got[2].tobytes() == want[2].tobytes(), label
                assert st["n_edges"] == want[0].shape[0], label
                check_route(st, world, bounds, n, slab_bytes, label)
            if thr == nothing:
                assert want[0].shape == (0,)
        if kind == "tail":
            src, tgt, val = multi.fill_edges(metric, 0.5, as_distance=as_distance)
            assert (src.tolist(), tgt.tolist()) == ([n - 2], [n - 1]) and bounds[-2] <= n - 1      # the last device's pair, alone
        if kind == "chain":
            src, tgt, _ = multi.fill_edges(metric, 0.7 if as_distance else 0.3, as_distance=as_distance)
            assert np.array_equal(tgt, np.arange(1, n)) and np.array_equal(src, np.arange(n - 1))     # one edge per target, every stretch


# ---- the dense fixtures, directly ------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_three_devices_equal_the_dense_fixture(multis, small_packed, synth200_packed, name, metric):
    from phamclust_amd.matrix import NearestNeighbors, SparseEdges, SymMatrix
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    names, distances, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
    matrix = SymMatrix.from_condensed(names, distances, is_distance=True)
    multi = multis(3)
    multi.upload(packed)
    forced = 8 * 1000
    for k in (5, 64):
        want = NearestNeighbors.from_dense(matrix, k)
        for slab_bytes in (0, forced):
            nbr, val, st = multi.fill_nearest(metric, k, slab_bytes=slab_bytes, want_stats=True)
            assert np.array_equal(nbr, want.indices) and np.array_equal(val, want.weights), (name, metric, k, slab_bytes)
            assert st["k"] == min(k, n - 1) and st["n_devices"] == 3
    every = SparseEdges.from_dense(matrix, 2.0)
    some = thresholds(distances, True)
    for thr in some:
        want = SparseEdges.from_dense(matrix, thr)
        assert 0 < len(want) < packed.n_pairs
        for slab_bytes in (0, forced):
            src, tgt, val = multi.fill_edges(metric, thr, slab_bytes=slab_bytes)
            assert np.array_equal(src, want.source) and np.array_equal(tgt, want.target) and np.array_equal(val, want.weight), (name, metric, thr)
        for strict in (True, False) if thr == some[-1] else (True,):       # the most frequent value: where '<' and '<=' part
            labels, st = multi.fill_components(metric, thr, strict=strict, slab_bytes=forced, want_stats=True)
            assert np.array_equal(labels, every.components(thr, strict=strict)), (name, metric, thr, strict)
            assert st["n_edges"] == int((distances < thr).sum() if strict else (distances <= thr).sum())


# ---- state and loans -------------------------------------------------------------------------------------
def test_state_and_loans(ctx, multis, small_packed):
    """A dense multi fill before and after each of the three is unchanged (either leaves the contexts as the other needs them);
    arrays are copies unless borrowed, and a loan ends with the next call; another context is not touched."""
    from phamclust_amd.hip import HipLibraryError
    n = small_packed.n_genomes
    multi = multis(3)
    multi.upload(small_packed, residues=False)
    ctx.upload(small_packed)
    for metric in ("jc", "peq"):
        _, distances, _ = read_lower_triangle(golden_file(metric))
        single_nbr, single_val = ctx.fill_nearest(metric, 5)
        assert np.array_equal(multi.fill("jc", borrow=False), read_lower_triangle(golden_file("jc"))[1])
        nbr, val = multi.fill_nearest(metric, 5, slab_bytes=8 * 40)
        assert isinstance(nbr, np.ndarray) and nbr.flags.writeable and np.array_equal(nbr, single_nbr) and np.array_equal(val, single_val)
        assert np.array_equal(multi.fill("jc", borrow=False), read_lower_triangle(golden_file("jc"))[1])
        labels = multi.fill_components(metric, 0.75, slab_bytes=8 * 40)
        src, tgt, edge_val = multi.fill_edges(metric, 0.75, slab_bytes=8 * 40)
        assert np.array_equal(multi.fill("jc", borrow=False), read_lower_triangle(golden_file("jc"))[1])
        assert np.array_equal(nbr, single_nbr) and np.array_equal(val, single_val)                       # copies: later calls did not touch them
        assert np.array_equal(labels, ctx.fill_components(metric, 0.75))
        for g, w in zip((src, tgt, edge_val), ctx.fill_edges(metric, 0.75)):
            assert np.array_equal(g, w)
        # borrowed: good until the next call on the multi context, whichever it is
        lent_nbr, lent_val = multi.fill_nearest(metric, 5, borrow=True)
        assert np.array_equal(np.asarray(lent_nbr), single_nbr) and np.array_equal(np.asarray(lent_val), single_val)
        between = ctx.fill_nearest(metric, 7)                               # another context in between: neither side notices
        assert np.array_equal(np.asarray(lent_nbr), single_nbr)
        lent_labels = multi.fill_components(metric, 0.75, borrow=True)
        with pytest.raises(HipLibraryError):
            np.asarray(lent_nbr)
        assert np.array_equal(np.asarray(lent_labels), labels)
        lent_edges = multi.fill_edges(metric, 0.75, borrow=True)
        with pytest.raises(HipLibraryError):
            np.asarray(lent_labels)
        assert np.array_equal(np.asarray(lent_edges[2]), edge_val)
        assert np.array_equal(multi.fill(metric, borrow=False), distances)
        with pytest.raises(HipLibraryError):
            np.asarray(lent_edges[0])
        assert np.array_equal(ctx.fill_nearest(metric, 7)[0], between[0]) and np.array_equal(ctx.fill(metric), distances)
        assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride()


def test_each_kind_keeps_its_own_times(ctx, multis, small_packed):
    """An edge-list, a components and a nearest fill in turn on ONE context, each with stats and over several slabs: afterwards
    pc_last_edge_times, pc_last_component_times and pc_last_nearest_times each still report exactly the pair their own call's stats
    carried.  The three calls time their passes with the same events of the context; a later call of another kind must not
    overwrite an earlier one's times.  The same sequence on two contexts of device 0 gives the single context's results."""
    slab_bytes = 8 * 40
    ctx.upload(small_packed)

    def sequence(on):
        *edges, edge_st = on.fill_edges("jc", 0.75, slab_bytes=slab_bytes, want_stats=True)
        labels, cc_st = on.fill_components("jc", 0.75, slab_bytes=slab_bytes, want_stats=True)
        nbr, val, nn_st = on.fill_nearest("jc", 5, slab_bytes=slab_bytes, want_stats=True)
        assert min(edge_st["n_slabs"], cc_st["n_slabs"], nn_st["n_slabs"]) > 1
        return (*edges, labels, nbr, val), (edge_st, cc_st, nn_st)

    single, (edge_st, cc_st, nn_st) = sequence(ctx)
    for call, st, first, second in (("pc_last_edge_times", edge_st, "ms_compact", "ms_d2h"), ("pc_last_component_times", cc_st, "ms_union", "ms_labels"),
                                    ("pc_last_nearest_times", nn_st, "ms_select", "ms_finish")):
        a, b = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
        assert getattr(ctx._lib, call)(ctx._h, ctypes.byref(a), ctypes.byref(b)) == 0, call
        print(call, a.value, b.value, st[first], st[second])
        assert (a.value, b.value) == (st[first], st[second]) and a.value > 0.0, call
    multi = multis(2)
    multi.upload(small_packed, residues=False)
    several, _ = sequence(multi)
    for g, w in zip(several, single):
        assert g.dtype == w.dtype and np.array_equal(g, w)


# ---- refusals --------------------------------------------------------------------------------------------
def test_refusals_through_the_binding(multis, small_packed):
    from phamclust_amd import hip
    from phamclust_amd.hip import HipLibraryError, _f64p, _i32p
    with hip.MultiContext([0, 0]) as fresh:                                 # before an upload
        for call in (lambda: fresh.fill_nearest("jc", 5), lambda: fresh.fill_components("jc", 0.5), lambda: fresh.fill_edges("jc", 0.5)):
            with pytest.raises(HipLibraryError, match="status -3"):
                call()
    multi = multis(2)
    multi.upload(small_packed, residues=False)
    n = small_packed.n_genomes
    with pytest.raises(HipLibraryError, match="status -1"):
        multi.fill_nearest("jc", 0)
    with pytest.raises(HipLibraryError, match="status -4"):
        multi.fill_nearest("jc", 65)
    for bad in (dict(threshold=float("nan")), dict(slab_bytes=-1)):
        with pytest.raises(HipLibraryError, match="status -1"):
            multi.fill_edges("jc", **dict(dict(threshold=0.5), **bad))
        with pytest.raises(HipLibraryError, match="status -1"):
            multi.fill_components("jc", **dict(dict(threshold=0.5), **bad))
    with pytest.raises(HipLibraryError, match="status -1"):
        multi.fill_nearest("jc", 5, slab_bytes=-8)
    lib, h = multi._lib, multi._h

    def nearest(metric=1, k=5, nbr_out=True, slab_bytes=0):
        pn, pv, kk, ns = _i32p(), _f64p(), ctypes.c_int32(7), ctypes.c_int32(7)
        rc = lib.pc_multi_fill_nearest(h, metric, 1, k, slab_bytes, ctypes.byref(pn) if nbr_out else None, ctypes.byref(pv), ctypes.byref(kk),
                                       ctypes.byref(ns), None)
        return rc, bool(pn), bool(pv), kk.value, ns.value

    assert nearest(nbr_out=False) == (-1, False, False, 0, 0)              # a NULL output pointer: the others nulled
    assert nearest(metric=9) == (-1, False, False, 0, 0) and nearest(k=0) == (-1, False, False, 0, 0)
    assert nearest(k=65) == (-4, False, False, 0, 0) and nearest(slab_bytes=-8) == (-1, False, False, 0, 0)
    assert nearest(metric=5) == (-3, False, False, 0, 0)                   # peq before the residues (the raw call uploads nothing)
    assert nearest() == (0, True, True, 5, 2) and nearest(k=64) == (0, True, True, n - 1, 2)

    def components(labels_out=True, thr=0.5, slab_bytes=0):
        pl, nc, ne, ns = _i32p(), ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int32(7)
        rc = lib.pc_multi_fill_components(h, 1, 1, thr, 1, slab_bytes, ctypes.byref(pl) if labels_out else None, ctypes.byref(nc), ctypes.byref(ne),
                                          ctypes.byref(ns), None)
        return rc, bool(pl), nc.value, ne.value, ns.value

    assert components(labels_out=False) == (-1, False, 0, 0, 0) and components(thr=float("nan")) == (-1, False, 0, 0, 0)
    assert components(slab_bytes=-1) == (-1, False, 0, 0, 0) and components()[:2] == (0, True)

    def edges(src_out=True, n_out=True, thr=0.5):
        ps, pt, pv, ne, ns = _i32p(), _i32p(), _f64p(), ctypes.c_int64(7), ctypes.c_int32(7)
        rc = lib.pc_multi_fill_edges(h, 1, 1, thr, 0, ctypes.byref(ps) if src_out else None, ctypes.byref(pt), ctypes.byref(pv),
                                     ctypes.byref(ne) if n_out else None, ctypes.byref(ns), None)
        return rc, bool(ps), bool(pt), bool(pv), ne.value if n_out else None, ns.value

    assert edges(src_out=False) == (-1, False, False, False, 0, 0) and edges(n_out=False) == (-1, False, False, False, None, 0)
    assert edges(thr=float("nan")) == (-1, False, False, False, 0, 0) and edges()[:4] == (0, True, True, True)
    assert lib.pc_multi_fill_nearest(None, 1, 1, 5, 0, None, None, None, None, None) == -1
    bounds = np.zeros(3, dtype=np.int32)
    assert lib.pc_multi_last_stretches(h, bounds.ctypes.data_as(_i32p)) == 0 and bounds[0] == 0 and bounds[2] == n
    assert lib.pc_multi_last_stretches(h, None) == -1 and lib.pc_multi_last_slab_times(None, None, None) == -1
    # after the refusals the devices serve as before
    want = read_lower_triangle(golden_file("jc"))[1]
    assert np.array_equal(multi.fill("jc", borrow=False), want)


# ---- command line ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag,target", [(["--nearest", "5"], "nearest_jc.tsv"), (["--adjacency-only"], "pairwise_jc_adjacency.tsv"),
                                         (["--components-only"], "components_jc.tsv")])
def test_flags_with_gpus_write_the_same_bytes(tmp_path, monkeypatch, native_built, flag, target):
    from phamclust_amd.scripts.phamclust import main
    one, two = tmp_path / "one", tmp_path / "two"
    main([os.path.join(GOLDEN, "small_input.tsv"), str(one), "-m", "jc"] + flag)
    monkeypatch.setenv("PHAMCLUST_GPU_IDS", "0,0")
    monkeypatch.setenv("PHAMCLUST_FORCE_GPUS", "1")
    main([os.path.join(GOLDEN, "small_input.tsv"), str(two), "-m", "jc", "--gpus", "2"] + flag)
    assert (two / target).read_bytes() == (one / target).read_bytes() and (one / target).stat().st_size > 0
    log_one, log_two = (one / "phamclust.log").read_text(), (two / "phamclust.log").read_text()
    assert "on 1 GPU in" in log_one and "2 GPUs" not in log_one
    assert "on 2 GPUs (targets 0.." in log_two and "on 1 GPU in" not in log_two and "one-GPU call" not in log_two
    assert "--gpus 2: PHAMCLUST_FORCE_GPUS is set" in log_two
