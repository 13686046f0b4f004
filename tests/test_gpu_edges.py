"""The edge-list fill (pc_fill_edges / Context.fill_edges / edges_de_novo / --adjacency-only) on the GPU (run with ``-m gpu``).

The expected edges always come from a DENSE condensed vector -- a golden file the live reference wrote, the oracle's fill, or (aai /
peq across slabs) the same context's whole fill, which the rest of the suite pins: ``(s, t) = triu_indices``, the predicate as a
mask, ``lexsort((s, t))``.  The assertion is exact: sources and targets equal, values bit-equal, in order.  A compaction that is
wrong at a chunk or wave seam, at a short row (the first targets lie many to a chunk) or at a tie (``<=`` against ``<``) fails
here; so does a slab walk that leaves the context sharded."""

import json
import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, SET_METRICS, golden_file, read_lower_triangle, synth200_file

pytestmark = pytest.mark.gpu


def expected_edges(condensed, n, thr, as_distance):
    s, t = np.triu_indices(n, k=1)
    keep = np.flatnonzero((condensed <= thr) if as_distance else (condensed >= thr))
    keep = keep[np.lexsort((s[keep], t[keep]))]
    return s[keep].astype(np.int32), t[keep].astype(np.int32), np.asarray(condensed)[keep]


def assert_edges(got, want, label):
    for name, g, w in zip(("src", "tgt", "val"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.shape, w.shape)
        assert np.array_equal(g, w), (label, name)
    assert got[2].tobytes() == want[2].tobytes(), (label, "bits")


def thresholds(dense, as_distance):
    """Distances: 0.999999, 0.75 and the most frequent value below 1 (a tie wherever the fixture has one, tests/test_edges_host.py);
    similarities: the same three from the other side -- 0.000001, 0.25 and the most frequent value above 0."""
    inner = dense[dense < 1.0] if as_distance else dense[dense > 0.0]
    values, counts = np.unique(inner, return_counts=True)
    return [0.999999 if as_distance else 0.000001, 0.75 if as_distance else 0.25, float(values[np.argmax(counts)])]


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


_SYNTH = {}


def synth_packed(n):
    """synth(n, 5000), name-sorted and packed, once per size."""
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    if n not in _SYNTH:
        _SYNTH[n] = pack_genomes(sorted(synth_genomes(n, 5000), key=lambda g: g.name))
    return _SYNTH[n]


_ORACLE = {}


def oracle_fill(name, packed, metric, as_distance):
    from oracle import oracle
    key = (name, metric, bool(as_distance))
    if key not in _ORACLE:
        _ORACLE[key] = np.asarray(oracle.fill(packed, metric, as_distance))
        _ORACLE[key].flags.writeable = False
    return _ORACLE[key]


def hand_built(n, kind):
    """n genomes of 4 genes each: "identical" -- the same phams and translations everywhere; "disjoint" -- no pham shared."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:03d}")
        for j in range(4):
            g.add(f"p{j}" if kind == "identical" else f"p{k}_{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        genomes.append(g)
    return pack_genomes(genomes)


# ---- 1: the fixtures the live reference wrote --------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_edges_equal_the_dense_fixture(ctx, small_packed, synth200_packed, name, metric):
    from phamclust_amd.hip import Context
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    _, distances, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
    forced = 8 * 300                                              # synth200: every target above 300 / t a slab of few targets, ~60 slabs; small: one
    n_forced = len(Context.edge_slabs(n, forced)) - 1
    assert n_forced == 1 if name == "small" else n_forced >= 50
    ctx.upload(packed)
    for as_distance in (True, False):
        dense = distances if as_distance else oracle_fill(name, packed, metric, False)
        for thr in thresholds(dense, as_distance):
            want = expected_edges(dense, n, thr, as_distance)
            assert 0 < want[0].shape[0] < packed.n_pairs
            for slab_bytes, n_slabs in ((0, 1), (forced, n_forced)):
                *got, st = ctx.fill_edges(metric, thr, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
                label = (name, metric, as_distance, thr, slab_bytes)
                assert_edges(got, want, label)
                assert st["n_edges"] == want[0].shape[0] and st["n_slabs"] == n_slabs, label
                assert st["n_pairs"] == n * (n - 1) // 2, label


# ---- 2: chunk and wave seams ----------------------------------------------------------------------
@pytest.mark.parametrize("metric", SET_METRICS)
def test_edges_across_chunk_seams(ctx, metric):
    """synth(600, 5000): 179,700 pairs, 44 chunks of 4,096; the slab cut moves every seam."""
    from phamclust_amd.hip import Context
    packed = synth_packed(600)
    n = packed.n_genomes
    dense = oracle_fill("synth600", packed, metric, True)
    ctx.upload(packed, residues=False)
    slab_bytes = 8 * 60000
    n_slabs = len(Context.edge_slabs(n, slab_bytes)) - 1
    assert n_slabs >= 3
    for thr in (0.999999, 0.75):
        want = expected_edges(dense, n, thr, True)
        assert 0 < want[0].shape[0] < packed.n_pairs
        for sb, ns in ((0, 1), (slab_bytes, n_slabs), (8 * 4097, len(Context.edge_slabs(n, 8 * 4097)) - 1)):
            *got, st = ctx.fill_edges(metric, thr, slab_bytes=sb, want_stats=True)
            assert_edges(got, want, (metric, thr, sb))
            assert st["n_slabs"] == ns and st["n_pairs"] == packed.n_pairs and st["n_chunks"] == ns


# ---- 3: degenerate fills --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "af", "peq"])
def test_every_pair_and_no_pair(ctx, metric):
    n = 70
    s, t = np.triu_indices(n, k=1)
    order = np.lexsort((s, t))
    ctx.upload(hand_built(n, "identical"))
    for slab_bytes in (0, 8 * 100):
        src, tgt, val = ctx.fill_edges(metric, 0.0, slab_bytes=slab_bytes)
        assert src.shape[0] == 2415 and np.array_equal(src, s[order]) and np.array_equal(tgt, t[order]) and not val.any()
        src, tgt, val = ctx.fill_edges(metric, 1.0, as_distance=False, slab_bytes=slab_bytes)
        assert src.shape[0] == 2415 and np.array_equal(src, s[order]) and np.array_equal(tgt, t[order]) and (val == 1.0).all()
    ctx.upload(hand_built(n, "disjoint"))
    for slab_bytes in (0, 8 * 100):
        src, tgt, val, st = ctx.fill_edges(metric, 0.999999, slab_bytes=slab_bytes, want_stats=True)
        assert src.shape == tgt.shape == val.shape == (0,) and st["n_edges"] == 0 and st["n_pairs"] == 2415
        assert (src.dtype, tgt.dtype, val.dtype) == (np.int32, np.int32, np.float64)
    src, tgt, val = ctx.fill_edges(metric, 1.0)                    # d <= 1: all of them again, at distance 1
    assert src.shape[0] == 2415 and (val == 1.0).all()


def test_one_and_two_genomes(ctx):
    for n in (1, 2):
        ctx.upload(hand_built(n, "identical"))
        for metric in ("gcs", "peq"):
            src, tgt, val, st = ctx.fill_edges(metric, 0.5, want_stats=True)
            assert st["n_pairs"] == n - 1 and st["n_edges"] == n - 1
            assert src.tolist() == [0][: n - 1] and tgt.tolist() == [1][: n - 1] and val.tolist() == [0.0][: n - 1]
            src, tgt, val = ctx.fill_edges(metric, 0.5, as_distance=False, slab_bytes=8)
            assert src.tolist() == [0][: n - 1] and val.tolist() == [1.0][: n - 1]


def test_thresholds_beyond_the_values(ctx, small_packed):
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    for metric in ("jc", "peq"):
        _, distances, _ = read_lower_triangle(golden_file(metric))
        src, tgt, val = ctx.fill_edges(metric, -1.0)
        assert src.shape == tgt.shape == val.shape == (0,)
        assert_edges(ctx.fill_edges(metric, 2.0), expected_edges(distances, n, 2.0, True), (metric, 2.0))
        assert ctx.fill_edges(metric, 2.0)[0].shape[0] == n * (n - 1) // 2
        assert ctx.fill_edges(metric, 2.0, as_distance=False)[0].shape[0] == 0
        assert ctx.fill_edges(metric, float("inf"))[0].shape[0] == n * (n - 1) // 2


# ---- 4: aai / peq across slabs against the same context's dense fill ---------------------------------
@pytest.mark.parametrize("metric", ["peq", "aai", "aai_ppos"])
def test_aligned_metrics_across_slabs(ctx, metric):
    from phamclust_amd.hip import Context
    packed = synth_packed(400)
    n = packed.n_genomes
    ctx.upload(packed)
    dense = ctx.fill(metric)
    slab_bytes = 8 * 30000
    n_slabs = len(Context.edge_slabs(n, slab_bytes)) - 1
    assert n_slabs == 3
    for thr in (0.999999, 0.75):
        want = expected_edges(dense, n, thr, True)
        assert 0 < want[0].shape[0] < packed.n_pairs
        for sb, ns in ((0, 1), (slab_bytes, n_slabs)):
            *got, st = ctx.fill_edges(metric, thr, slab_bytes=sb, want_stats=True)
            assert_edges(got, want, (metric, thr, sb))
            assert st["n_slabs"] == ns and st["n_chunks"] >= ns and st["n_pairs"] == packed.n_pairs and st["n_alignments"] > 0


# ---- 5: the context afterwards ----------------------------------------------------------------------
def test_state_restored_and_errors(ctx, small_packed):
    from phamclust_amd.hip import HipLibraryError
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    for metric in ("jc", "peq"):
        _, distances, _ = read_lower_triangle(golden_file(metric))
        lent = ctx.fill(metric, borrow=True)
        assert np.array_equal(lent, distances)
        ctx.fill_edges(metric, 0.75, slab_bytes=8 * 40)
        with pytest.raises(HipLibraryError):                      # the loan ended with the edge-list fill
            lent.sum()
        assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride()
        t_rank, t_lbase = ctx.shard_table()
        assert not t_rank.any() and np.array_equal(t_lbase, np.arange(n) * (np.arange(n) - 1) // 2)
        assert np.array_equal(ctx.fill(metric), distances)
    # a borrowed edge list ends with the next fill
    src, tgt, val = ctx.fill_edges("jc", 0.75, borrow=True)
    assert np.array_equal(np.asarray(val), expected_edges(read_lower_triangle(golden_file("jc"))[1], n, 0.75, True)[2])
    ctx.fill("jc")
    with pytest.raises(HipLibraryError):
        np.asarray(src)
    # argument and state errors, by code
    for bad in (dict(threshold=float("nan")), dict(slab_bytes=-1)):
        with pytest.raises(HipLibraryError, match="status -1"):
            ctx.fill_edges("jc", **dict(dict(threshold=0.5), **bad))
    ctx.set_shard(1, 3)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):
            ctx.fill_edges("jc", 0.75)
    finally:
        ctx.set_shard(0, 1)
    assert_edges(ctx.fill_edges("jc", 0.75), expected_edges(read_lower_triangle(golden_file("jc"))[1], n, 0.75, True), "after the refusal")
    ctx.upload(small_packed, residues=False)
    lib, h = ctx._lib, ctx._h
    import ctypes
    from phamclust_amd.hip import _f64p, _i32p
    ps, pt, pv, ne, ns = _i32p(), _i32p(), _f64p(), ctypes.c_int64(7), ctypes.c_int32(7)
    assert lib.pc_fill_edges(h, 5, 1, 0.5, 0, ctypes.byref(ps), ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(ne), ctypes.byref(ns), None) == -3   # peq before the residues
    assert ne.value == 0 and ns.value == 0 and not ps
    assert lib.pc_fill_edges(h, 1, 1, 0.5, 0, None, ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(ne), ctypes.byref(ns), None) == -1
    assert lib.pc_fill_edges(h, 9, 1, 0.5, 0, ctypes.byref(ps), ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(ne), ctypes.byref(ns), None) == -1
    assert lib.pc_fill_edges(h, 1, 1, 0.75, 0, ctypes.byref(ps), ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(ne), ctypes.byref(ns), None) == 0 and ne.value > 0


def test_a_refusal_inside_the_walk_restores_the_shard(ctx):
    """A slab's fill refused in the middle of the walk: three genomes, one with an empty translation in a shared pham, slab_bytes=8 --
    two slabs, target 2 gets a range of its own.  peq is refused with the library's data status (-5) from inside the first slab's
    fill, while that slab's one-target shard is in force; afterwards the context is the unsharded one it was: three pairs, the
    dense jc fill unchanged, and an edge-list fill over the same two slabs agrees with it."""
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
        ctx.fill_edges("peq", 0.75, slab_bytes=8)
    assert ctx.shard_pairs() == 3 == ctx.shard_stride()
    assert np.array_equal(ctx.fill("jc"), before)
    for thr in (2.0, 0.25):                                       # every pair; the pairs of equal genomes only
        *got, st = ctx.fill_edges("jc", thr, slab_bytes=8, want_stats=True)
        assert st["n_slabs"] == 2 and st["n_pairs"] == 3
        assert_edges(got, expected_edges(before, 3, thr, True), ("after the refusal", thr))


# ---- 6: the reference's own file --------------------------------------------------------------------
def test_adjacency_only_run_writes_the_reference_file(tmp_path, small_genomes, native_built):
    from phamclust_amd import cli
    from phamclust_amd.matrix import matrix_de_novo, matrix_to_adjacency
    from phamclust_amd.scripts.phamclust import main
    fixture = json.load(open(os.path.join(GOLDEN, "pipeline_jc", "tree.json")))
    out = tmp_path / "out"
    main([os.path.join(GOLDEN, "small_input.tsv"), str(out), "-m", "jc", "--adjacency-only"])
    written = out / "pairwise_jc_adjacency.tsv"
    as_map = lambda text: {frozenset(l.split("\t")[:2]): l.split("\t")[2] for l in text.splitlines()}      # noqa: E731
    assert as_map(written.read_text()) == as_map(fixture["files"]["pairwise_jc_adjacency.tsv"])
    dense = tmp_path / "dense.tsv"
    matrix_to_adjacency(matrix_de_novo(small_genomes, cli.METRICS["jc"], 1).invert(), dense, skip_zero=True)
    assert written.read_bytes() == dense.read_bytes()
    files = sorted(p.relative_to(out).as_posix() for p in out.rglob("*") if p.is_file() and "01_genomes" not in p.as_posix())
    assert files == ["pairwise_jc_adjacency.tsv", "phamclust.log"]                 # no dense cache, no clusters
    log = (out / "phamclust.log").read_text()
    assert "slab(s)" in log and "pairs" in log
    # --edge-thresh: the same file filtered to similarity >= 0.25
    out2 = tmp_path / "out2"
    main([os.path.join(GOLDEN, "small_input.tsv"), str(out2), "-m", "jc", "--adjacency-only", "--edge-thresh", "0.25"])
    kept = [l for l in dense.read_text().splitlines(keepends=True) if float(l.split("\t")[2]) >= 0.25]
    assert (out2 / "pairwise_jc_adjacency.tsv").read_text() == "".join(kept) and 0 < len(kept) < len(dense.read_text().splitlines())
