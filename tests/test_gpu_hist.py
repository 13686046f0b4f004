"""The distribution fill (pc_fill_hist / Context.fill_hist / MultiContext.fill_hist / Context.fill_rows_hist / distribution_de_novo /
distribution_extend / --distribution-only / --distribution) on the GPU with the release library and real metrics (run with ``-m gpu``).

The expected histogram always comes from the same upload's whole fill, which the rest of the suite pins: ``np.bincount`` of the
millionths of ``Context.fill``.  Every comparison is exact.  A pair counted twice or dropped at a chunk or slab seam shows in the
bins' sum; a state that does not survive from slab to slab, a class taken for the other, a reversal that is off by one bin or a merge
that counts a stretch twice fails here."""

import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN

pytestmark = pytest.mark.gpu

MILLION = 1000000
BINS = MILLION + 1


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def micros(values):
    k = np.rint(np.asarray(values) * 1.0e6).astype(np.int64)
    assert np.array_equal(k / 1.0e6, np.asarray(values))
    return k


def pair_ends(n):
    """(s, t) of the condensed (scipy) order of n genomes."""
    s, t = np.triu_indices(n, k=1)
    return s, t


@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("collection", ["small", "synth200"])
def test_fill_hist_is_the_bincount_of_the_whole_fill(ctx, request, collection, metric):
    from phamclust_amd import hip
    from phamclust_amd.matrix import PairDistribution
    packed = request.getfixturevalue("small_packed" if collection == "small" else "synth200_packed")
    ctx.upload(packed, residues=metric in hip.NEEDS_RESIDUES)
    n = ctx.n_genomes
    pairs = n * (n - 1) // 2
    k = micros(ctx.fill(metric))
    want = np.bincount(k, minlength=BINS).astype(np.int64)[None, :]
    cuts = (0, 8 * (pairs // 3 + 1), 8 * 5000) if collection == "synth200" else (0, 8 * 100)
    assert collection == "small" or pairs > 4 * 4096
    for slab_bytes in cuts:
        got, st = ctx.fill_hist(metric, slab_bytes=slab_bytes, want_stats=True)
        assert got.dtype == np.int64 and np.array_equal(got, want), (slab_bytes,)
        assert st["hist_pairs"] == pairs and st["n_classes"] == 1 and (st["n_slabs"] > 1) == (slab_bytes > 0)
        assert st["ms_pass"] > 0.0 and st["ms_finish"] > 0.0
    back = ctx.fill_hist(metric, as_distance=False)
    assert np.array_equal(back, want[:, ::-1])                               # the inverted matrix's histogram: every millionth's complement
    # what the histogram answers without a second fill: the edge count at any threshold
    dist = PairDistribution.from_hist(got, is_distance=True)
    ordered = np.sort(k)
    for threshold in (float(ordered[len(ordered) // 10]) / 1.0e6, float(ordered[len(ordered) // 2]) / 1.0e6, 0.999999):
        src, _, _, est = ctx.fill_edges(metric, threshold, want_stats=True)
        assert dist.count_within(threshold) == est["n_edges"] == src.shape[0], threshold
    sim = PairDistribution.from_hist(back, is_distance=False)
    assert sim == dist.inverted() and sim.count_within(0.000001) == int((k <= 999999).sum())
    # the components at a threshold as the partition: class 0 is exactly the pairs a groups fill delivers
    roots = ctx.fill_components(metric, float(ordered[len(ordered) // 4]) / 1.0e6 + 1e-6)
    _, label = np.unique(roots, return_inverse=True)
    label = label.astype(np.int32)
    groups = [np.flatnonzero(label == a).astype(np.int32) for a in range(int(label.max()) + 1)]
    inside = np.concatenate(ctx.fill_groups(metric, groups) or [np.empty(0)])
    s, t = pair_ends(n)
    same = label[s] == label[t]
    for slab_bytes in cuts[:2]:
        split = ctx.fill_hist(metric, label, slab_bytes=slab_bytes)
        assert split.shape == (2, BINS) and np.array_equal(split.sum(axis=0), want[0])
        assert int(split[0].sum()) == inside.shape[0] == int(same.sum()) == sum(len(g) * (len(g) - 1) // 2 for g in groups)
        assert np.array_equal(split[0], np.bincount(micros(inside), minlength=BINS))
        assert np.array_equal(split[1], np.bincount(k[~same], minlength=BINS))
    assert np.array_equal(ctx.fill_hist(metric, label, as_distance=False), split[:, ::-1])
    # the rows form: the last genomes against a histogram of the first
    new = 3 if collection == "small" else 17
    old_pairs = (n - new) * (n - new - 1) // 2
    among_old = (s < n - new) & (t < n - new)
    rows = np.arange(n - new, n, dtype=np.int32)
    for group in (None, label):
        if group is None:
            seed = np.bincount(k[among_old], minlength=BINS).astype(np.int64)[None, :]
            whole = want
        else:
            seed = np.stack([np.bincount(k[among_old & same], minlength=BINS), np.bincount(k[among_old & ~same], minlength=BINS)]).astype(np.int64)
            whole = split
        assert int(seed.sum()) == old_pairs
        for slab_bytes in (0, 8 * n * 2):
            got, st = ctx.fill_rows_hist(metric, rows, group=group, seed=seed, slab_bytes=slab_bytes, want_stats=True)
            assert np.array_equal(got, whole) and st["hist_pairs"] == pairs and st["n_slabs"] == (1 if slab_bytes == 0 else (new + 1) // 2)
        assert np.array_equal(ctx.fill_rows_hist(metric, rows, group=group, seed=seed[:, ::-1], as_distance=False), whole[:, ::-1])
        assert np.array_equal(ctx.fill_rows_hist(metric, rows, group=group), whole - seed)
        assert np.array_equal(ctx.fill_rows_hist(metric, [], group=group, seed=np.ascontiguousarray(whole)), whole)     # no row: the seed comes back


def test_fill_hist_on_several_contexts_is_the_single_context_s(ctx, synth200_packed, native_built):
    from phamclust_amd import hip
    ctx.upload(synth200_packed, residues=True)
    n = ctx.n_genomes
    label = (np.arange(n) % 7).astype(np.int32)
    for world in (2, 3):
        with hip.MultiContext([0] * world) as multi:
            multi.upload(synth200_packed, residues=True)
            for metric in ("jc", "peq"):
                for group in (None, label):
                    want = ctx.fill_hist(metric, group)
                    got, st = multi.fill_hist(metric, group, slab_bytes=8 * 3000, want_stats=True)
                    assert np.array_equal(got, want) and st["n_devices"] == world and st["hist_pairs"] == n * (n - 1) // 2
                    assert np.array_equal(multi.fill_hist(metric, group, as_distance=False), want[:, ::-1])


def test_loans_and_refusals(ctx, small_packed):
    from phamclust_amd import hip
    ctx.upload(small_packed, residues=False)
    lent = ctx.fill_hist("jc", borrow=True)
    kept = np.array(lent)
    again = ctx.fill_hist("gcs", borrow=True)                                 # the next call ends the loan
    with pytest.raises(Exception):
        lent.sum()
    assert int(np.array(again).sum()) == int(kept.sum()) == ctx.n_pairs
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_hist: genome 2 has label 9, outside \[0, 3\)"):
        ctx.fill_hist("jc", np.where(np.arange(ctx.n_genomes) == 2, 9, 0).astype(np.int32), 3)
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_hist: metric 77"):
        ctx._check(ctx._lib.pc_fill_hist(ctx._h, 77, 1, None, 0, 0, None, None, None, None, None))
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_hist: an output pointer is NULL"):
        ctx._check(ctx._lib.pc_fill_hist(ctx._h, 1, 1, None, 0, 0, None, None, None, None, None))
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_rows_hist: rows must be strictly ascending"):
        ctx.fill_rows_hist("jc", [3, 3])
    with pytest.raises(ValueError, match="seed must be 1 x"):
        ctx.fill_rows_hist("jc", [3], seed=np.zeros((2, BINS), dtype=np.int64))
    ctx.set_shard(0, 2)
    try:
        with pytest.raises(hip.HipLibraryError, match=r"pc_fill_hist: context is sharded"):
            ctx.fill_hist("jc")
    finally:
        ctx.set_shard(0, 1)
    assert np.array_equal(ctx.fill_hist("jc"), kept)


# ---- the routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_distribution_de_novo_and_extend(native_built, small_genomes, metric):
    from phamclust_amd import matrix as M
    from phamclust_amd.cli import METRICS
    func = METRICS[metric]
    names = [g.name for g in small_genomes]
    dense = M.matrix_de_novo(small_genomes, func, 1)
    groups = [names[0:9], names[9:10], names[10:23]]
    for part in (None, groups):
        want = M.PairDistribution.from_dense(dense, part)
        found = M.distribution_de_novo(small_genomes, func, groups=part)
        assert found == want and found.nodes == names and M.LAST_FILL["n_gpus"] == 1
        assert found.statistics == want.statistics and (part is not None or abs(found.mean - dense.statistics[0]) < 1e-12)
        sim = M.distribution_de_novo(small_genomes, func, groups=part, as_distance=False)
        assert sim == want.inverted()
        # grown from a stored distribution of the genomes but three
        new = {names[2], names[10], names[22]}
        old_genomes = [g for g in small_genomes if g.name not in new]
        old_groups = None if part is None else [[x for x in group if x not in new] for group in part]
        for as_distance in (True, False):
            stored = M.distribution_de_novo(old_genomes, func, groups=old_groups, as_distance=as_distance)
            grown = M.distribution_extend(stored, small_genomes, func, groups=part)
            assert grown == (want if as_distance else want.inverted()) and grown.nodes == names
            assert M.LAST_FILL["rows"] == 3
    # a stored distribution of another metric: a refilled value falls in no bin it populates
    other = METRICS["gcs" if metric == "jc" else "aai"]
    stale = M.distribution_de_novo(old_genomes, other)
    with pytest.raises(ValueError, match=r"distribution_extend: pair \('"):
        M.distribution_extend(stale, small_genomes, func)
    # every genome new: the de novo route
    empty = M.PairDistribution(([], []), nodes=[])
    assert M.distribution_extend(empty, small_genomes, func) == M.PairDistribution.from_dense(dense)


def test_distribution_de_novo_on_two_devices(native_built, small_genomes, monkeypatch):
    from phamclust_amd import matrix as M
    from phamclust_amd.cli import METRICS
    one = M.distribution_de_novo(small_genomes, METRICS["pocp"])
    monkeypatch.setenv("PHAMCLUST_GPU_IDS", "0,0")
    two = M.distribution_de_novo(small_genomes, METRICS["pocp"])
    assert two == one and M.LAST_FILL["n_gpus"] == 2


# ---- command line ------------------------------------------------------------------------------------------------------------
FILES = ("pairwise_jc_distribution.tsv", "pairwise_jc_distribution_summary.tsv")


def test_distribution_only_writes_the_same_bytes_on_two_devices(tmp_path, monkeypatch, native_built):
    from phamclust_amd.matrix import PairDistribution, SymMatrix
    from phamclust_amd.scripts.phamclust import main
    from conftest import golden_file, read_lower_triangle
    tsv = os.path.join(GOLDEN, "small_input.tsv")
    one, two = tmp_path / "one", tmp_path / "two"
    main([tsv, str(one), "-m", "jc", "--distribution-only", "-e", "0.3"])
    assert sorted(p.name for p in one.iterdir() if p.is_file()) == sorted(FILES + ("phamclust.log",))
    names, condensed, _ = read_lower_triangle(golden_file("jc"))
    matrix = SymMatrix.from_condensed(names, condensed, is_distance=True)
    matrix.invert()
    want = PairDistribution.from_dense(matrix)
    assert PairDistribution.from_file(str(one / FILES[0]), is_distance=False) == want
    summary = dict(line.split("\t") for line in (one / FILES[1]).read_text().splitlines())
    assert summary["n"] == "253" and summary["mean"] == repr(want.mean) and summary["median"] == f"{want.median:.6f}"
    assert summary["pairs_at_edge_thresh_0.300000"] == str(want.count_within(0.3)) and summary["pairs_at_clu_thresh_0.250000"] == str(want.count_within(0.25))
    monkeypatch.setenv("PHAMCLUST_GPU_IDS", "0,0")
    monkeypatch.setenv("PHAMCLUST_FORCE_GPUS", "1")
    main([tsv, str(two), "-m", "jc", "--distribution-only", "-e", "0.3", "--gpus", "2"])
    for name in FILES:
        assert (two / name).read_bytes() == (one / name).read_bytes() and (one / name).stat().st_size > 0
    assert "on 1 GPU in" in (one / "phamclust.log").read_text() and "on 2 GPUs (targets 0.." in (two / "phamclust.log").read_text()


def test_distribution_add_on_is_the_same_on_the_dense_route_and_without_the_matrix(tmp_path, native_built):
    import json
    from phamclust_amd.matrix import PairDistribution
    from phamclust_amd.scripts.phamclust import main
    fixture = json.load(open(os.path.join(GOLDEN, "pipeline_jc", "tree.json")))
    argv = ["-m", "jc", "-k", str(fixture["k_min"]), "-t", "1", "-nl", "single", "-cl", "single", "--distribution"]
    dense, sparse = tmp_path / "dense", tmp_path / "no_matrix"
    main([os.path.join(GOLDEN, "small_input.tsv"), str(dense)] + argv)
    main([os.path.join(GOLDEN, "small_input.tsv"), str(sparse), "--no-matrix"] + argv)
    for name in FILES:
        assert (dense / name).read_bytes() == (sparse / name).read_bytes() and (dense / name).stat().st_size > 0
    found = PairDistribution.from_file(str(dense / FILES[0]), is_distance=False)
    assert found.partitioned and found.n_pairs == 253
    summary = dict(line.split("\t") for line in (dense / FILES[1]).read_text().splitlines())
    assert summary["within_pairs"] == str(found.within.n_pairs) and summary["best_separation"] == f"{found.best_separation()[0]:.6f}"
    assert summary["within_beyond_clu_thresh_0.250000"] == str(found.separation(0.25)[0])
    assert "distribution fill" in (sparse / "phamclust.log").read_text() and "the dense matrix" in (dense / "phamclust.log").read_text()
