"""The components fill (pc_fill_components / Context.fill_components / components_de_novo / hierarchical_clustering_de_novo /
--components-only) on the GPU (run with ``-m gpu``).

The expected labels always come from a DENSE vector -- a golden file the live reference wrote, the oracle's fill, or (aai / peq
beyond the fixtures) the same context's whole fill, which the rest of the suite pins -- through
``SparseEdges.from_dense(...).components(...)``, the host statement tests/test_components_host.py holds to the reference's
single-linkage clustering.  The assertion is exact: ``np.array_equal(labels, want)`` with ``n_components`` and ``n_edges``; a
non-strict run's ``n_edges`` must also be ``fill_edges``' count.  A union that loses a hook under contention, a parent[] that does
not survive from one slab to the next, a pair indexed wrongly at a chunk seam or a short row, or ``<`` taken for ``<=`` at a tie
fails here; so does a walk that leaves the context sharded."""

import ctypes
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


class Dense:
    """A dense condensed vector and its every-pair edge list: the expected labels and counts of any threshold come from it."""

    def __init__(self, condensed, n, as_distance=True):
        from phamclust_amd.matrix import SparseEdges, SymMatrix
        self.condensed, self.n, self.as_distance = np.asarray(condensed), n, as_distance
        matrix = SymMatrix.from_condensed([f"n{k:05d}" for k in range(n)], self.condensed, is_distance=as_distance)
        self.edges = SparseEdges.from_dense(matrix, 2.0 if as_distance else -1.0)
        assert len(self.edges) == n * (n - 1) // 2

    def labels(self, thr, strict=True):
        return self.edges.components(thr, strict=strict)

    def passing(self, thr, strict=True):
        v = self.condensed
        if self.as_distance:
            return int((v < thr).sum() if strict else (v <= thr).sum())
        return int((v > thr).sum() if strict else (v >= thr).sum())


def check(ctx, metric, dense, thr, strict, slab_bytes, n_slabs=None, label=None):
    """One fill held to the dense vector: labels, n_components, n_edges (and the slab count where the caller knows it)."""
    label = label or (metric, dense.as_distance, thr, strict, slab_bytes)
    want = dense.labels(thr, strict)
    labels, st = ctx.fill_components(metric, thr, as_distance=dense.as_distance, strict=strict, slab_bytes=slab_bytes, want_stats=True)
    assert labels.dtype == np.int32 and labels.shape == (dense.n,), label
    assert np.array_equal(labels, want), label
    assert st["n_components"] == int((want == np.arange(dense.n)).sum()), label
    assert st["n_edges"] == dense.passing(thr, strict), label
    assert st["n_pairs"] == dense.n * (dense.n - 1) // 2, label
    if n_slabs is not None:
        assert st["n_slabs"] == n_slabs, label
    return labels, st


_SYNTH = {}


def synth_packed(n):
    """synth(n, 5000), name-sorted and packed, once per size."""
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    if n not in _SYNTH:
        _SYNTH[n] = pack_genomes(sorted(synth_genomes(n, 5000), key=lambda g: g.name))
    return _SYNTH[n]


_ORACLE = {}


def oracle_dense(name, packed, metric, as_distance=True):
    from oracle import oracle
    key = (name, metric, bool(as_distance))
    if key not in _ORACLE:
        _ORACLE[key] = Dense(oracle.fill(packed, metric, as_distance), packed.n_genomes, as_distance)
    return _ORACLE[key]


def hand_built(n, kind):
    """n genomes: "identical" -- the same 4 phams and translations everywhere; "disjoint" -- no pham shared; "chain" -- genome k
    holds phams p{k} and p{k+1}, so only neighbours share one (each pair of neighbours the same way: one value)."""
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


# ---- 1: the fixtures the live reference wrote --------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_components_equal_the_dense_fixture(ctx, small_packed, synth200_packed, name, metric):
    from phamclust_amd.hip import Context
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    _, distances, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
    forced = 8 * 300                                  # synth200: >= 50 slabs, so components span slabs and parent[] must persist; small: one
    n_forced = len(Context.edge_slabs(n, forced)) - 1
    assert n_forced == 1 if name == "small" else n_forced >= 50
    # an aligned metric's slab is a plan + align + reduce of its own (>= 50 of them per multi-slab fill): one height keeps the case at seconds
    heights = merge_heights(distances, 12 if metric in SET_METRICS else 1)
    assert len(heights) >= 1
    ctx.upload(packed)
    for as_distance in (True, False):
        dense = Dense(distances, n) if as_distance else oracle_dense(name, packed, metric, False)
        parted = 0
        for d in [0.4, 0.75, 0.999999] + heights:
            thr = d if as_distance else round(1.0 - d, 6)
            for strict in (True, False):
                for slab_bytes, n_slabs in ((0, 1), (forced, n_forced)):
                    _, st = check(ctx, metric, dense, thr, strict, slab_bytes, n_slabs, (name, metric, as_distance, thr, strict, slab_bytes))
                if not strict:
                    assert st["n_edges"] == ctx.fill_edges(metric, thr, as_distance=as_distance, want_stats=True)[3]["n_edges"]
            parted += not np.array_equal(dense.labels(thr, True), dense.labels(thr, False))
        if as_distance:                               # every merge height is a value of the matrix that '<' and '<=' answer differently
            assert parted >= len(heights), (name, metric)


# ---- 2: chunk seams -------------------------------------------------------------------------------
# what the oracle's synth(600, 5000) jc matrix holds: (components, largest) of {d < thr}
SYNTH600_JC = {0.6: (290, 27), 0.75: (15, 40)}


@pytest.mark.parametrize("metric", SET_METRICS)
def test_components_across_chunk_seams(ctx, metric):
    """synth(600, 5000): 179,700 pairs, 44 chunks of 4,096; the slab cut moves every seam."""
    from phamclust_amd.hip import Context
    packed = synth_packed(600)
    n = packed.n_genomes
    dense = oracle_dense("synth600", packed, metric)
    ctx.upload(packed, residues=False)
    for thr in (0.6, 0.75):
        sizes = np.bincount(dense.labels(thr))
        sizes = sizes[sizes > 0]
        assert 1 < sizes.shape[0] < n and sizes.max() > 1                        # not trivial
        if metric == "jc":
            assert (sizes.shape[0], int(sizes.max())) == SYNTH600_JC[thr]
        for sb in (0, 8 * 60000, 8 * 4097):
            ns = 1 if sb == 0 else len(Context.edge_slabs(n, sb)) - 1
            assert sb == 0 or ns >= 3
            _, st = check(ctx, metric, dense, thr, True, sb, ns)
            assert st["n_chunks"] == ns
        check(ctx, metric, dense, thr, False, 8 * 4097)


# ---- 3: aai / peq across slabs against the same context's dense fill ----------------------------------
SYNTH400_PEQ = {0.4: (371, 11), 0.6: (18, 40), 0.75: (10, 40)}


@pytest.mark.parametrize("metric", ["peq", "aai", "aai_ppos"])
def test_aligned_metrics_across_slabs(ctx, metric):
    from phamclust_amd.hip import Context
    packed = synth_packed(400)
    n = packed.n_genomes
    ctx.upload(packed)
    dense = Dense(ctx.fill(metric), n)
    slab_bytes = 8 * 30000
    assert len(Context.edge_slabs(n, slab_bytes)) - 1 == 3
    for thr in (0.4, 0.6, 0.75):
        if metric == "peq":
            sizes = np.bincount(dense.labels(thr))
            assert (int((sizes > 0).sum()), int(sizes.max())) == SYNTH400_PEQ[thr]
        for sb, ns in ((0, 1), (slab_bytes, 3)):
            _, st = check(ctx, metric, dense, thr, True, sb, ns)
            assert st["n_chunks"] >= ns and st["n_alignments"] > 0
    check(ctx, metric, dense, 0.6, False, slab_bytes, 3)


# ---- 4: shapes that stress the union -----------------------------------------------------------------
@pytest.mark.parametrize("n", [70, 600])
def test_every_pair_in_one_component(ctx, n):
    """Identical genomes: every pair passes, every hook aims at genome 0 -- the most contended union there is."""
    ctx.upload(hand_built(n, "identical"))
    pairs = n * (n - 1) // 2
    for metric in ("jc", "peq") if n == 70 else ("jc",):
        for slab_bytes in (0, 8 * 100 if n == 70 else 8 * 4097):
            labels, st = ctx.fill_components(metric, 0.5, slab_bytes=slab_bytes, want_stats=True)
            assert not labels.any() and st["n_components"] == 1 and st["n_edges"] == pairs
            labels, st = ctx.fill_components(metric, 0.0, strict=False, slab_bytes=slab_bytes, want_stats=True)       # d <= 0
            assert not labels.any() and st["n_components"] == 1 and st["n_edges"] == pairs
            labels, st = ctx.fill_components(metric, 0.0, slab_bytes=slab_bytes, want_stats=True)                     # d < 0: nothing
            assert np.array_equal(labels, np.arange(n)) and st["n_components"] == n and st["n_edges"] == 0
            labels, st = ctx.fill_components(metric, 1.0, as_distance=False, strict=False, slab_bytes=slab_bytes, want_stats=True)
            assert not labels.any() and st["n_edges"] == pairs


def test_no_pair_passes(ctx):
    n = 70
    ctx.upload(hand_built(n, "disjoint"))
    for metric in ("jc", "af", "peq"):
        for slab_bytes in (0, 8 * 100):
            labels, st = ctx.fill_components(metric, 0.999999, slab_bytes=slab_bytes, want_stats=True)
            assert np.array_equal(labels, np.arange(n)) and labels.dtype == np.int32
            assert st["n_edges"] == 0 and st["n_components"] == n and st["n_pairs"] == 2415
    labels, st = ctx.fill_components("jc", 1.0, strict=False, want_stats=True)       # d <= 1: every pair, at distance 1
    assert not labels.any() and st["n_edges"] == 2415


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_chain(ctx, metric):
    """300 genomes, only neighbours related, all at one value: one component from exactly 299 edges -- a tree of depth N if
    nothing shortens it -- and at that value itself '<' gives 300 components where '<=' gives one."""
    n = 300
    packed = hand_built(n, "chain")
    dense = oracle_dense("chain300", packed, metric)
    s, t = np.triu_indices(n, k=1)
    near = dense.condensed[t - s == 1]
    value = float(near[0])
    assert (near == value).all() and value < 0.7 and (dense.condensed[t - s > 1] == 1.0).all()
    if metric == "jc":
        assert value == 0.666667
    ctx.upload(packed)
    for slab_bytes in (0, 8 * 300):
        labels, st = check(ctx, metric, dense, 0.7, True, slab_bytes)
        assert not labels.any() and st["n_edges"] == n - 1 and st["n_components"] == 1
        labels, st = check(ctx, metric, dense, value, True, slab_bytes)
        assert st["n_components"] == n and st["n_edges"] == 0
        labels, st = check(ctx, metric, dense, value, False, slab_bytes)
        assert st["n_components"] == 1 and st["n_edges"] == n - 1


def test_one_and_two_genomes(ctx):
    for n in (1, 2):
        ctx.upload(hand_built(n, "identical"))
        for metric in ("gcs", "peq"):
            labels, st = ctx.fill_components(metric, 0.5, want_stats=True)
            assert labels.tolist() == [0] * n and st["n_components"] == 1 and st["n_edges"] == n - 1 and st["n_pairs"] == n - 1
            labels, st = ctx.fill_components(metric, 0.0, slab_bytes=8, want_stats=True)          # d < 0
            assert labels.tolist() == list(range(n)) and st["n_components"] == n and st["n_edges"] == 0


def test_thresholds_beyond_the_values(ctx, small_packed):
    n = small_packed.n_genomes
    pairs = n * (n - 1) // 2
    ctx.upload(small_packed)
    for metric in ("jc", "peq"):
        dense = Dense(read_lower_triangle(golden_file(metric))[1], n)
        for thr, passing in ((-1.0, 0), (2.0, pairs), (float("inf"), pairs)):
            for strict in (True, False):
                labels, st = check(ctx, metric, dense, thr, strict, 0)
                assert st["n_edges"] == passing and st["n_components"] == (1 if passing else n)
        labels, st = ctx.fill_components(metric, 2.0, as_distance=False, want_stats=True)          # sim > 2: nothing
        assert np.array_equal(labels, np.arange(n)) and st["n_edges"] == 0
        labels, st = ctx.fill_components(metric, float("-inf"), as_distance=False, want_stats=True)
        assert not labels.any() and st["n_edges"] == pairs


# ---- 5: determinism ------------------------------------------------------------------------------
def test_labels_do_not_depend_on_the_races(ctx, synth200_packed):
    ctx.upload(synth200_packed, residues=False)
    dense = Dense(read_lower_triangle(synth200_file("jc"))[1], synth200_packed.n_genomes)
    first, _ = check(ctx, "jc", dense, 0.75, True, 0)
    for k in range(4):
        again = ctx.fill_components("jc", 0.75, slab_bytes=0 if k % 2 else 8 * 300)
        assert np.array_equal(again, first)


# ---- 6: the context afterwards ----------------------------------------------------------------------
def test_state_restored_and_errors(ctx, small_packed):
    from phamclust_amd.hip import HipLibraryError, _i32p
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    for metric in ("jc", "peq"):
        _, distances, _ = read_lower_triangle(golden_file(metric))
        lent = ctx.fill(metric, borrow=True)
        assert np.array_equal(lent, distances)
        ctx.fill_components(metric, 0.75, slab_bytes=8 * 40)
        with pytest.raises(HipLibraryError):                      # the loan ended with the components fill
            lent.sum()
        assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride()
        t_rank, t_lbase = ctx.shard_table()
        assert not t_rank.any() and np.array_equal(t_lbase, np.arange(n) * (np.arange(n) - 1) // 2)
        assert np.array_equal(ctx.fill(metric), distances)
    # borrowed labels end with the next fill
    dense = Dense(read_lower_triangle(golden_file("jc"))[1], n)
    labels = ctx.fill_components("jc", 0.75, borrow=True)
    assert np.array_equal(np.asarray(labels), dense.labels(0.75))
    ctx.fill("jc")
    with pytest.raises(HipLibraryError):
        np.asarray(labels)
    # argument and state errors, by code
    for bad in (dict(threshold=float("nan")), dict(slab_bytes=-1)):
        with pytest.raises(HipLibraryError, match="status -1"):
            ctx.fill_components("jc", **dict(dict(threshold=0.5), **bad))
    ctx.set_shard(1, 3)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):
            ctx.fill_components("jc", 0.75)
    finally:
        ctx.set_shard(0, 1)
    check(ctx, "jc", dense, 0.75, True, 0, label="after the refusal")
    ctx.upload(small_packed, residues=False)
    lib, h = ctx._lib, ctx._h

    def call(metric, labels_out=True, thr=0.5, slab_bytes=0):
        pl, nc, ne, ns = _i32p(), ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int32(7)
        rc = lib.pc_fill_components(h, metric, 1, thr, 1, slab_bytes, ctypes.byref(pl) if labels_out else None, ctypes.byref(nc), ctypes.byref(ne),
                                    ctypes.byref(ns), None)
        return rc, bool(pl), nc.value, ne.value, ns.value

    assert call(5) == (-3, False, 0, 0, 0)                        # peq before the residues
    assert call(1, labels_out=False) == (-1, False, 0, 0, 0)
    assert call(9) == (-1, False, 0, 0, 0)
    assert call(-1) == (-1, False, 0, 0, 0)
    assert call(1, thr=float("nan")) == (-1, False, 0, 0, 0)
    assert call(1, slab_bytes=-8) == (-1, False, 0, 0, 0)
    rc, lent_out, nc, ne, ns = call(1, thr=0.75)
    assert rc == 0 and lent_out and nc == int((dense.labels(0.75) == np.arange(n)).sum()) and ne == dense.passing(0.75) and ns == 1
    a, b = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.pc_last_component_times(h, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0      # no stats asked
    _, st = ctx.fill_components("jc", 0.75, want_stats=True)
    assert st["ms_union"] > 0.0 and st["ms_labels"] > 0.0


def test_a_refusal_inside_the_walk_restores_the_shard(ctx):
    """A slab's fill refused in the middle of the walk: three genomes, one with an empty translation in a shared pham, slab_bytes=8 --
    two slabs, target 2 gets a range of its own.  peq is refused with the library's data status (-5) from inside the first slab's
    fill, while that slab's one-target shard is in force; afterwards the context is the unsharded one it was: three pairs, the
    dense jc fill unchanged, and a components fill over the same two slabs agrees with it."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.hip import HipLibraryError
    from phamclust_amd.pack import pack_genomes
    empty, other, third = Genome("e1"), Genome("e2"), Genome("e3")
    empty.add("p1", "")
    other.add("p1", "MK")
    third.add("p1", "MKV"); third.add("p2", "MA")
    ctx.upload(pack_genomes([empty, other, third]))
    before = ctx.fill("jc")
    assert before.shape == (3,)
    with pytest.raises(HipLibraryError, match="status -5.*empty translation"):
        ctx.fill_components("peq", 0.75, slab_bytes=8)
    assert ctx.shard_pairs() == 3 == ctx.shard_stride()
    assert np.array_equal(ctx.fill("jc"), before)
    for thr in (2.0, float(before.max())):                        # every pair; strictly below the largest distance
        check(ctx, "jc", Dense(before, 3), thr, True, 8, n_slabs=2)


# ---- 7: above the C-ABI ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_components_de_novo_gives_the_single_linkage_groups(small_genomes, native_built, metric):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    from phamclust_amd.clustering import hierarchical_clustering
    dense = M.matrix_de_novo(small_genomes, cli.METRICS[metric], 1)
    for eps in (0.4, 0.75):
        found = M.components_de_novo(small_genomes, cli.METRICS[metric], eps)
        assert found.groups() == [part.nodes for part in hierarchical_clustering(dense, "single", eps=eps)]
        assert M.LAST_FILL["n_components"] == found.n_components and M.LAST_FILL["metric"] == metric and M.LAST_FILL["n_slabs"] == 1
    sliced = M.components_de_novo(small_genomes, cli.METRICS[metric], 0.75, slab_bytes=8 * 40)
    assert np.array_equal(sliced.labels, found.labels) and M.LAST_FILL["n_slabs"] > 1


@pytest.mark.parametrize("metric", ["jc", "peq"])
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_clustering_de_novo_equals_the_dense_route(small_genomes, native_built, name, metric):
    from phamclust_amd import cli
    from phamclust_amd.clustering import hierarchical_clustering, hierarchical_clustering_de_novo
    from phamclust_amd.matrix import matrix_de_novo
    from phamclust_amd.synth import synth_genomes
    genomes = small_genomes if name == "small" else sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:200]
    func = cli.METRICS[metric]
    dense = matrix_de_novo(genomes, func, 1)
    for linkage in ("single", "average", "complete"):
        for eps in (0.4, 0.75):
            want = hierarchical_clustering(dense, linkage, eps=eps)
            got = hierarchical_clustering_de_novo(genomes, func, linkage, eps)
            assert [p.nodes for p in got] == [p.nodes for p in want], (name, metric, linkage, eps)
            for a, b in zip(got, want):
                assert np.array_equal(a.to_ndarray(), b.to_ndarray()), (name, metric, linkage, eps)


def test_components_only_run(tmp_path, small_genomes, native_built):
    from phamclust_amd import cli
    from phamclust_amd.matrix import components_de_novo
    from phamclust_amd.scripts.phamclust import main
    names = [g.name for g in small_genomes]
    for k, extra in enumerate(([], ["--edge-thresh", "0.25"])):
        out = tmp_path / f"out{k}"
        main([os.path.join(GOLDEN, "small_input.tsv"), str(out), "-m", "jc", "--components-only"] + extra)
        files = sorted(p.relative_to(out).as_posix() for p in out.rglob("*") if p.is_file() and "01_genomes" not in p.as_posix())
        assert files == ["components_jc.tsv", "phamclust.log"]                       # no matrix, no adjacency file, no clusters
        rows = [line.split("\t") for line in (out / "components_jc.tsv").read_text().splitlines()]
        assert [r[0] for r in rows] == names
        groups = components_de_novo(small_genomes, cli.METRICS["jc"], 0.75 if extra else 1.0).groups()
        number = {name: str(i) for i, group in enumerate(groups, start=1) for name in group}
        assert [r[1] for r in rows] == [number[name] for name in names]
        log = (out / "phamclust.log").read_text()
        assert f"{len(groups):,} components" in log and "slab(s)" in log and f"the largest of {len(groups[0]):,}" in log
    assert len(groups) > 1
