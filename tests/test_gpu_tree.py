"""The tree fill (pc_fill_tree / pc_multi_fill_tree / Context.fill_tree / MultiContext.fill_tree / tree_de_novo / --tree) on the GPU
(run with ``-m gpu``).

The expected tree always comes from a DENSE vector -- a golden file the live reference wrote, the oracle's fill, or the same
context's whole fill, which the rest of the suite pins -- through ``SingleLinkageTree.from_dense``, the host statement
tests/test_tree_host.py holds to scipy's and scikit-learn's single linkage.  Every assertion is exact: ``np.array_equal`` on ``src``,
``tgt`` and the bits of ``val``.  A round that loses a minimum under contention, a hook that lets a cycle form among tied edges, a
forest that does not survive from one slab to the next, a pair indexed wrongly at a chunk seam, a merge of two devices' forests that
drops an edge, or a walk that leaves the context sharded fails here."""

import ctypes
import math
import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, SET_METRICS, golden_file, read_lower_triangle, synth200_file

pytestmark = pytest.mark.gpu


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


def tree_of(condensed, n, as_distance=True):
    """``SingleLinkageTree.from_dense`` of a condensed vector over n nodes."""
    from phamclust_amd.matrix import SingleLinkageTree, SymMatrix
    matrix = SymMatrix.from_condensed([f"n{k:05d}" for k in range(n)], np.asarray(condensed), is_distance=as_distance)
    return SingleLinkageTree.from_dense(matrix)


_WANT = {}


def fixture_tree(name, packed, metric, as_distance):
    """The expected tree of a committed fixture: from the golden distances, or (similarities) from the oracle's fill.  Computed once."""
    key = (name, metric, bool(as_distance))
    if key not in _WANT:
        if as_distance:
            _, values, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
        else:
            from oracle import oracle
            values = oracle.fill(packed, metric, False)
        _WANT[key] = tree_of(values, packed.n_genomes, as_distance)
    return _WANT[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check(got, want, label):
    """(src, tgt, val) of a fill held to a SingleLinkageTree."""
    src, tgt, val = got[:3]
    assert src.dtype == np.int32 and tgt.dtype == np.int32 and val.dtype == np.float64, label
    assert np.array_equal(src, want.source), label
    assert np.array_equal(tgt, want.target), label
    assert same_bits(val, want.weight), label


def rounds_of(n):
    return max(1, math.ceil(math.log2(n))) if n > 1 else 0


def check_stats(st, n, n_slabs, label):
    assert st["n_edges"] == max(n - 1, 0) and st["n_pairs"] == n * (n - 1) // 2, label
    if n_slabs is not None:
        assert st["n_slabs"] == n_slabs, label
    assert 0 <= st["live_rounds"] <= st["launched_rounds"] <= st["n_slabs"] * rounds_of(n), label
    if n > 1:
        assert st["live_rounds"] >= 1, label


def hand_built(n, kind):
    """n genomes: "identical" -- the same 4 phams and translations everywhere; "disjoint" -- no pham shared; "chain" -- genome k
    holds phams p{k} and p{k+1}, so only neighbours share one (each pair of neighbours the same way: one value).  The collections
    of tests/test_gpu_components.py, rebuilt here."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        if kind == "chain":
            g.add(f"p{k}", "MKTAYIAKQRQISFVKSHFSRQ")
            g.add(f"p{k + 1}", "MKTAYLAKQRQISWVKSHFARQ")
        else:
            for j in range(4):
                g.add(f"p{j}" if kind == "identical" else f"p{k}_{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        genomes.append(g)
    return pack_genomes(genomes)


def merge_heights(condensed, most):
    """Up to ``most`` evenly spaced single-linkage merge heights: values of the matrix at which '<' and '<=' part."""
    from scipy.cluster.hierarchy import linkage
    heights = np.unique(linkage(np.asarray(condensed), "single")[:, 2])
    return heights[np.unique(np.linspace(0, heights.shape[0] - 1, min(most, heights.shape[0])).round().astype(int))].tolist()


# ---- 1, 2: the fixtures the live reference wrote; the components fill on the same uploads ----------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_tree_equals_the_dense_fixture(ctx, small_packed, synth200_packed, name, metric):
    from phamclust_amd.hip import Context
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    forced = 8 * 300                                  # synth200: >= 50 slabs, so the forest must persist and be re-merged; small: one
    n_forced = len(Context.edge_slabs(n, forced)) - 1
    assert n_forced == 1 if name == "small" else n_forced >= 50
    ctx.upload(packed)
    for as_distance in (True, False):
        want = fixture_tree(name, packed, metric, as_distance)
        for slab_bytes, n_slabs in ((0, 1), (forced, n_forced)):
            label = (name, metric, as_distance, slab_bytes)
            *got, st = ctx.fill_tree(metric, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
            check(got, want, label)
            check_stats(st, n, n_slabs, label)
    # against the components fill: an independent, already pinned GPU path
    want = fixture_tree(name, packed, metric, True)
    _, distances, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
    heights = merge_heights(distances, 12 if metric in SET_METRICS else 1)
    assert len(heights) >= 1
    for thr in heights:
        for strict in (True, False):
            assert np.array_equal(want.cut(thr, strict), ctx.fill_components(metric, thr, strict=strict)), (name, metric, thr, strict)


# ---- 3: hand-built collections -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 65, 100, 300])
@pytest.mark.parametrize("kind", ["identical", "disjoint", "chain"])
def test_hand_built_collections(ctx, kind, n):
    """identical / disjoint: every value ties, the tree is the star at genome 0 -- any Boruvka without the strict order builds
    cycles here.  chain: the path, all its edges at one value.  n = 100 is 4,950 pairs: it crosses the 4,096-element chunk.  Each
    whole and with one target per slab (n - 1 slabs with pairs)."""
    from phamclust_amd.hip import Context
    ctx.upload(hand_built(n, kind))
    for metric in ("jc", "peq"):
        dense = ctx.fill(metric)
        want = tree_of(dense, n)
        if kind == "chain":
            assert want.source.tolist() == list(range(n - 1)) and want.target.tolist() == list(range(1, n))
            assert (want.weight == want.weight[0]).all() and want.weight[0] < 1.0
        else:
            assert want.source.tolist() == [0] * (n - 1) and want.target.tolist() == list(range(1, n))
            assert (want.weight == (0.0 if kind == "identical" else 1.0)).all()
        for slab_bytes in (0, 8):
            label = (kind, n, metric, slab_bytes)
            *got, st = ctx.fill_tree(metric, slab_bytes=slab_bytes, want_stats=True)
            check(got, want, label)
            check_stats(st, n, len(Context.edge_slabs(n, 8)) - 1 if slab_bytes else 1, label)
            if slab_bytes:
                assert st["n_slabs"] == n - 1, label                        # one target per slab (targets 0 and 1 share the first)
        similar = tree_of(ctx.fill(metric, as_distance=False), n, as_distance=False)
        check(ctx.fill_tree(metric, as_distance=False, slab_bytes=8 * 70), similar, (kind, n, metric, "similarity"))
        assert np.array_equal(similar.source, want.source) and np.array_equal(similar.target, want.target)


# ---- 4: a slab with real contention ---------------------------------------------------------------------
def test_one_large_slab(ctx):
    """synth(2000, 5000), jc, one slab of ~2 million pairs: the heights against scipy's single linkage of the dense fill, cuts
    against the components fill, every edge's value against the dense vector (a full host Kruskal is not run at this size)."""
    from scipy.cluster.hierarchy import linkage
    from phamclust_amd.matrix import SingleLinkageTree
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    packed = pack_genomes(sorted(synth_genomes(2000, 5000), key=lambda g: g.name))
    n = packed.n_genomes
    ctx.upload(packed, residues=False)
    dense = ctx.fill("jc")
    src, tgt, val, st = ctx.fill_tree("jc", want_stats=True)
    check_stats(st, n, 1, "synth2000")
    assert (src < tgt).all() and tgt.max() < n
    s64, t64 = src.astype(np.int64), tgt.astype(np.int64)
    assert same_bits(val, dense[s64 * n - s64 * (s64 + 1) // 2 + (t64 - s64 - 1)])
    assert np.array_equal(np.lexsort((src, tgt, val)), np.arange(n - 1))                 # delivered in the total order
    heights = linkage(dense, "single")[:, 2]
    assert same_bits(val, heights)
    tree = SingleLinkageTree([f"n{k:05d}" for k in range(n)], src, tgt, val)
    distinct = np.unique(heights)
    for thr in distinct[[distinct.shape[0] // 4, distinct.shape[0] // 2, (3 * distinct.shape[0]) // 4]].tolist():
        for strict in (True, False):
            assert np.array_equal(tree.cut(thr, strict), ctx.fill_components("jc", thr, strict=strict)), (thr, strict)


# ---- 5: the result is canonical --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_the_tree_depends_neither_on_the_cut_nor_on_the_devices(ctx, multis, synth200_packed, metric):
    from phamclust_amd.hip import Context, MultiContext
    packed = synth200_packed
    n = packed.n_genomes
    want = fixture_tree("synth200", packed, metric, True)
    ctx.upload(packed)
    for slab_bytes in (0, 8 * 5000, 8 * 300 if metric == "jc" else 8 * 1500):
        n_slabs = 1 if slab_bytes == 0 else len(Context.edge_slabs(n, slab_bytes)) - 1
        assert slab_bytes == 0 or n_slabs >= 4
        *got, st = ctx.fill_tree(metric, slab_bytes=slab_bytes, want_stats=True)
        check(got, want, (metric, slab_bytes))
        check_stats(st, n, n_slabs, (metric, slab_bytes))
    if metric == "jc":
        cost = np.arange(n, dtype=np.uint64)
    else:
        ctx.set_shard(0, 1, balanced=True)
        cost = ctx.target_costs() + np.arange(n, dtype=np.uint64) * np.uint64(2000)
        ctx.set_shard(0, 1)
    for world in (1, 2, 3, 5):
        multi = multis(world)
        multi.upload(packed, residues=False)                                   # the residues follow on demand, on every device
        bounds = MultiContext.slab_stretches(cost, world).tolist()
        for slab_bytes in (0, 8 * 1500):
            label = (metric, world, slab_bytes)
            *got, st = multi.fill_tree(metric, slab_bytes=slab_bytes, want_stats=True)
            check(got, want, label)
            assert st["n_edges"] == n - 1 and st["n_devices"] == world == len(st["per_device"]), label
            assert st["stretches"] == bounds and bounds[0] == 0 and bounds[-1] == n, label
            assert st["n_pairs"] == n * (n - 1) // 2 == sum(p["n_pairs"] for p in st["per_device"]), label
            for r, per in enumerate(st["per_device"]):
                a, b = bounds[r], bounds[r + 1]
                assert per["n_pairs"] == b * (b - 1) // 2 - a * (a - 1) // 2, (label, r)
            assert st["ms_exchange"] >= 0.0 and st["ms_merge"] >= 0.0, label
            if slab_bytes:
                cuts = sum(len(Context.chunk_plan(np.arange(a, b, dtype=np.uint64), slab_bytes // 8)) - 1 for a, b in zip(bounds, bounds[1:]) if b > a)
                assert st["n_slabs"] == cuts, label
        similar = fixture_tree("synth200", packed, metric, False) if metric == "jc" else None
        if similar is not None:
            check(multi.fill_tree(metric, as_distance=False, slab_bytes=8 * 1500), similar, (metric, world, "similarity"))


@pytest.mark.parametrize("kind,n", [("identical", 3), ("chain", 4), ("identical", 130)])
def test_more_contexts_than_targets_and_ties_across_devices(ctx, multis, kind, n):
    """Five contexts over 3 or 4 genomes: some stretches are empty and ship nothing.  130 identical genomes: every value ties, so
    across the devices' forests the order alone decides which edges stay."""
    packed = hand_built(n, kind)
    ctx.upload(packed)
    multi = multis(5)
    multi.upload(packed, residues=False)
    for metric in ("jc", "peq"):
        want = tree_of(ctx.fill(metric), n)
        for slab_bytes in (0, 8):
            *got, st = multi.fill_tree(metric, slab_bytes=slab_bytes, want_stats=True)
            check(got, want, (kind, n, metric, slab_bytes))
            bounds = st["stretches"]
            assert bounds[0] == 0 and bounds[-1] == n and all(a <= b for a, b in zip(bounds, bounds[1:]))
            if n < 5:
                assert any(a == b for a, b in zip(bounds, bounds[1:]))
            for r, per in enumerate(st["per_device"]):
                if bounds[r] == bounds[r + 1]:
                    assert not any(per.values()), (kind, n, metric, r)       # an empty stretch: zeros, nothing ran
        check(ctx.fill_tree(metric), want, (kind, n, metric, "single context"))


# ---- 6: refusals and the context afterwards -----------------------------------------------------------------
def test_one_and_no_genome(ctx, multis):
    for n in (1, 2):
        packed = hand_built(n, "identical")
        ctx.upload(packed)
        multi = multis(2)
        multi.upload(packed, residues=False)
        for metric in ("gcs", "peq"):
            for who in (ctx, multi):
                src, tgt, val, st = who.fill_tree(metric, slab_bytes=8, want_stats=True)
                assert src.tolist() == [0] * (n - 1) and tgt.tolist() == [1] * (n - 1) and val.tolist() == [0.0] * (n - 1)
                assert st["n_edges"] == n - 1 and st["n_pairs"] == n - 1


def test_state_restored_and_errors(ctx, small_packed):
    from phamclust_amd.hip import HipLibraryError, _f64p, _i32p
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    for metric in ("jc", "peq"):
        _, distances, _ = read_lower_triangle(golden_file(metric))
        lent = ctx.fill(metric, borrow=True)
        assert np.array_equal(lent, distances)
        ctx.fill_tree(metric, slab_bytes=8 * 40)
        with pytest.raises(HipLibraryError):                      # the loan ended with the tree fill
            lent.sum()
        assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride()
        t_rank, t_lbase = ctx.shard_table()
        assert not t_rank.any() and np.array_equal(t_lbase, np.arange(n) * (np.arange(n) - 1) // 2)
        assert np.array_equal(ctx.fill(metric), distances)        # a whole fill after a tree fill equals the one before it
    want = fixture_tree("small", small_packed, "jc", True)
    borrowed = ctx.fill_tree("jc", borrow=True)
    check([np.asarray(x) for x in borrowed], want, "borrowed")
    ctx.fill("jc")
    with pytest.raises(HipLibraryError):
        np.asarray(borrowed[2])
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_tree("jc", slab_bytes=-1)
    ctx.set_shard(1, 3)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):
            ctx.fill_tree("jc")
    finally:
        ctx.set_shard(0, 1)
    check(ctx.fill_tree("jc"), want, "after the refusal")
    ctx.upload(small_packed, residues=False)
    lib, h = ctx._lib, ctx._h

    def call(metric, handle=h, outs=(True, True, True), counts=True, slab_bytes=0):
        ps, pt, pv, ne, ns = _i32p(), _i32p(), _f64p(), ctypes.c_int32(7), ctypes.c_int32(7)
        rc = lib.pc_fill_tree(handle, metric, 1, slab_bytes, ctypes.byref(ps) if outs[0] else None, ctypes.byref(pt) if outs[1] else None,
                              ctypes.byref(pv) if outs[2] else None, ctypes.byref(ne) if counts else None, ctypes.byref(ns), None)
        return rc, bool(ps), bool(pt), bool(pv), ne.value if counts else 0, ns.value

    refused = (False, False, False, 0, 0)
    assert call(5) == (-3, *refused)                              # peq before the residues
    assert call(1, handle=None) == (-3, *refused)                 # no context: nothing uploaded
    assert call(9) == (-1, *refused) and call(-1) == (-1, *refused)
    assert call(1, slab_bytes=-8) == (-1, *refused)
    for k in range(3):
        assert call(1, outs=tuple(j != k for j in range(3))) == (-1, *refused)
    assert call(1, counts=False) == (-1, *refused)
    rc, a, b, c, ne, ns = call(1)
    assert rc == 0 and a and b and c and ne == n - 1 and ns == 1
    x, y = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.pc_last_tree_times(h, ctypes.byref(x), ctypes.byref(y)) == 0 and x.value == 0.0 and y.value > 0.0      # no stats asked: no events
    live, launched = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.pc_last_tree_rounds(h, ctypes.byref(live), ctypes.byref(launched)) == 0
    assert 1 <= live.value <= launched.value == rounds_of(n)
    assert lib.pc_last_tree_rounds(None, ctypes.byref(live), ctypes.byref(launched)) == -1
    *_, st = ctx.fill_tree("jc", want_stats=True)
    assert st["ms_rounds"] > 0.0 and st["ms_finish"] > 0.0
    fresh = type(ctx)(0)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):   # before upload
            fresh._check(lib.pc_fill_tree(fresh._h, 1, 1, 0, ctypes.byref(_i32p()), ctypes.byref(_i32p()), ctypes.byref(_f64p()),
                                          ctypes.byref(ctypes.c_int32(0)), ctypes.byref(ctypes.c_int32(0)), None))
    finally:
        fresh.close()


# ---- 7: above the C-ABI ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_tree_de_novo(small_genomes, small_packed, native_built, metric):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    from phamclust_amd.clustering import hierarchical_clustering
    want = fixture_tree("small", small_packed, metric, True)
    found = M.tree_de_novo(small_genomes, cli.METRICS[metric])
    check((found.source, found.target, found.weight), want, metric)
    assert found.nodes == [g.name for g in small_genomes] and found.is_distance
    assert M.LAST_FILL["n_edges"] == len(small_genomes) - 1 and M.LAST_FILL["metric"] == metric and M.LAST_FILL["n_slabs"] == 1
    sliced = M.tree_de_novo(small_genomes, cli.METRICS[metric], slab_bytes=8 * 40)
    check((sliced.source, sliced.target, sliced.weight), want, metric)
    assert M.LAST_FILL["n_slabs"] > 1
    dense = M.matrix_de_novo(small_genomes, cli.METRICS[metric], 1)
    for eps in (0.4, 0.75):
        assert M.Components(found.nodes, found.cut(eps)).groups() == [part.nodes for part in hierarchical_clustering(dense, "single", eps=eps)]
    assert found.leaves() == M._get_tree_order(dense) or len(set(found.weight.tolist())) < len(found)      # the reference's leaf order, ties aside


def test_tree_run(tmp_path, small_genomes, native_built):
    from phamclust_amd import cli
    from phamclust_amd.matrix import tree_de_novo
    from phamclust_amd.scripts.phamclust import main
    out = tmp_path / "out"
    main([os.path.join(GOLDEN, "small_input.tsv"), str(out), "-m", "jc", "--tree"])
    files = sorted(p.relative_to(out).as_posix() for p in out.rglob("*") if p.is_file() and "01_genomes" not in p.as_posix())
    assert files == ["phamclust.log", "tree_jc.tsv"]                           # no matrix, no adjacency file, no clusters
    rows = [line.split("\t") for line in (out / "tree_jc.tsv").read_text().splitlines()]
    found = tree_de_novo(small_genomes, cli.METRICS["jc"])
    assert len(rows) == len(small_genomes) - 1
    assert [(r[0], r[1]) for r in rows] == [(a, b) for a, b, _ in found]
    assert [r[2] for r in rows] == [f"{w:.6f}" for _, _, w in found.inverted()]
    log = (out / "phamclust.log").read_text()
    assert "edges of the single-linkage tree" in log and "slab(s)" in log and "wrote tree_jc.tsv" in log
