"""Every kernel that stages the presence bitmap, on collections that sit ON its 32-word chunk edges, and the walkers' rows / groups /
slab domains on the numeric-edge genomes (MI355X; run with ``-m gpu``).

The popcount tiles (k_set_popc, k_set_popc_ksplit) and the walkers (k_walk in its POCP / AF / COUNT / ENUM / AAI / PEQ modes,
k_walk_rows, k_walk_groups) stage 32 bitmap words per chunk.  tests/word_edge_cases.py builds collections of exactly 1, 31, 32, 33,
64, 65 and 97 words -- a final chunk of 31 words, of 32, of ONE word holding ONE pham --, with phams that many genomes share on bit
63 of each chunk's last word and bit 0 of the next chunk's first, and genomes whose phams all lie in the last word / in word 32
(tests/test_word_edges_host.py proves that on the CPU).  Every comparison here is ``np.array_equal`` against the oracle's whole
matrix, no tolerance: a lost bit, a skipped final chunk or a mask that forgets its 32nd word changes almost every pair.

The second half runs fill_rows, fill_groups, fill_edges and fill_components on the genomes of tests/golden/set_edges/ (65,535 /
65,536 copies of a pham, 1,023 / 1,024 genes, entries of 65,535 / 65,536 residues, empty translations), against the values the LIVE
reference wrote -- so far only the whole-fill families had met them."""

import numpy as np
import pytest

import set_kernel_cases as S
import word_edge_cases as WE
from test_gpu_components import Dense, check
from test_gpu_edges import assert_edges, expected_edges
from test_gpu_set_kernels import FORCED, _assert_launch, _edge_want, _set_knobs, _shard_columns

pytestmark = pytest.mark.gpu
SHAPES = pytest.mark.parametrize("shape", WE.SHAPES, ids=WE.shape_id)
SET_METRICS, ALIGNED = WE.SEVEN[:4], WE.SEVEN[4:]
# the families a fill can be forced onto and the metrics each exists for (pc_set_shape.hip): these must RUN when forced here
FAMILIES = FORCED + (("sparsecol", None),)
HAS_METRIC = {"popc": ("gcs", "jc", "pocp"), "sparse": ("pocp", "af"), "walker": ("pocp", "af"), "sparse64": SET_METRICS, "sparsecol": SET_METRICS}


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    _set_knobs()
    yield gpu_ctx
    _set_knobs()
    gpu_ctx.set_shard(0, 1)
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def first_difference(got, want, n):
    """(s, t, got, want) of the first pair at which two condensed vectors differ, or None."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if not bad.size:
        return None
    s, t = np.triu_indices(n, k=1)
    return int(s[bad[0]]), int(t[bad[0]]), float(got[bad[0]]), float(want[bad[0]]), int(bad.size)


def median_value(vector):
    """A threshold that OCCURS in the vector: its median element (so '<=' and '<' part)."""
    return float(np.sort(np.asarray(vector))[len(vector) // 2])


# ---- whole fills ------------------------------------------------------------------------------------------------------------
@SHAPES
def test_set_metric_families_whole_and_sharded(ctx, native_built, shape):
    """gcs / jc / pocp / af, both polarities: the selector's own choice, then every family forced (both popcount tiles, the 32 x 32
    and 64 x 64 sparse tiles, the walker, the column kernel) -- the family must run where the selector's host function admits it,
    and it must admit every family for the metrics it exists for --, then the same as both shards of a 2-rank deal, boustrophedon
    and cost-balanced."""
    import torch
    from phamclust_amd import hip
    packed = WE.collection(shape)
    n = packed.n_genomes
    stats = S.recount(packed)
    fields = S.selector_inputs(stats)
    want = {(m, d): WE.oracle_fill(shape, m, d) for m in SET_METRICS for d in (True, False)}
    stream = torch.cuda.current_stream().cuda_stream
    try:
        ctx.upload(packed, residues=False)
        ctx.set_shard(0, 1)
        for family, tile in ((None, None),) + FAMILIES:
            _set_knobs(PC_SET_KERNEL=family, PC_POPC_TILE=tile)
            ctx.set_shard(0, 1)
            for m in SET_METRICS:
                admitted = hip.Context.set_kernel_choice(m, forced=family, **fields)
                if family is not None and m in HAS_METRIC[family]:
                    assert admitted == family, (shape, family, m, admitted)
                for dist in (True, False):
                    got = ctx.fill(m, dist)
                    assert first_difference(got, want[(m, dist)], n) is None, (shape, family, tile, m, dist, ctx.last_set_kernel())
                    ran, launch = _assert_launch(ctx, stats, m)
                    assert ran == admitted == ctx.last_set_kernel() and (tile is None or ran != "popc" or launch["tile"] == tile)
            for balanced in S.DEALS:
                for rank in range(2):
                    ctx.set_shard(rank, 2, balanced=balanced)
                    t_rank, t_lbase = ctx.shard_table()
                    owned = np.flatnonzero(t_rank == rank)
                    for m in SET_METRICS:
                        buf = torch.full((max(ctx.shard_stride(), 1),), -1.0, dtype=torch.float64, device="cuda:0")
                        ctx.fill_shard_dev(m, True, buf.data_ptr(), stream, want_stats=False)
                        torch.cuda.synchronize()
                        ran, _ = _assert_launch(ctx, stats, m, owned)
                        assert family is None or m not in HAS_METRIC[family] or ran == family, (shape, family, m, rank, balanced, ran)
                        assert _shard_columns(want[(m, True)], n, t_rank, t_lbase, rank, buf.cpu().numpy()) is None, (shape, family, tile, m, rank, balanced)
    finally:
        _set_knobs()
        ctx.set_shard(0, 1)


@SHAPES
def test_aligned_metrics_whole(ctx, native_built, shape):
    """aai / peq / aai_ppos, both polarities: k_walk counts the alignments of every pair (COUNT), lays out their sort keys (ENUM)
    and reduces the best matches (AAI / PEQ) over the same staged chunks."""
    packed = WE.collection(shape)
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    for m in ALIGNED:
        for dist in (True, False):
            got, st = ctx.fill(m, dist, want_stats=True)
            assert first_difference(got, WE.oracle_fill(shape, m, dist), packed.n_genomes) is None, (shape, m, dist)
            assert st["n_alignments"] > 0 and st["n_pairs"] == packed.n_pairs


# ---- the rows and the groups walker -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metrics", [SET_METRICS, ALIGNED], ids=["sets", "aligned"])
@SHAPES
def test_rows_fill(ctx, native_built, shape, metrics):
    """k_walk_rows, all seven metrics, both polarities: the first row, the last, the rows around the 32-row tile edge, one query
    from each tile, the extra genomes, and all rows -- against the oracle's square, the diagonal preset."""
    packed = WE.collection(shape)
    n = packed.n_genomes
    ctx.upload(packed, residues=metrics is ALIGNED)
    ctx.set_shard(0, 1)
    for m in metrics:
        for dist in (True, False):
            want = WE.square(WE.oracle_fill(shape, m, dist), n, dist)
            for label, rows in WE.row_sets(shape).items():
                got = ctx.fill_rows(m, rows, dist)
                assert got.shape == (len(rows), n) and got.dtype == np.float64
                bad = np.argwhere(got != want[rows])
                assert not bad.size, (shape, m, dist, label, "first (row, genome)", rows[bad[0][0]], int(bad[0][1]), got[tuple(bad[0])], want[rows][tuple(bad[0])], len(bad))


@pytest.mark.parametrize("metrics", [SET_METRICS, ALIGNED], ids=["sets", "aligned"])
@SHAPES
def test_groups_fill(ctx, native_built, shape, metrics):
    """k_walk_groups, all seven metrics, both polarities: one group of everything (the whole vector), groups cut at positions 31,
    32 and 33 of the member list, forty random pairs, two overlapping groups, the extra genomes with three others."""
    packed = WE.collection(shape)
    n = packed.n_genomes
    ctx.upload(packed, residues=metrics is ALIGNED)
    ctx.set_shard(0, 1)
    families = WE.group_families(shape)
    for m in metrics:
        for dist in (True, False):
            flat = WE.oracle_fill(shape, m, dist)
            want = WE.square(flat, n, dist)
            for label, groups in families.items():
                got = ctx.fill_groups(m, groups, dist)
                assert len(got) == len(groups)
                for k, (group, values) in enumerate(zip(groups, got)):
                    assert values.dtype == np.float64 and values.shape == (len(group) * (len(group) - 1) // 2,)
                    assert np.array_equal(values, WE.condensed_of(want, group)), (shape, m, dist, label, k)
            assert first_difference(ctx.fill_groups(m, families["everything"], dist)[0], flat, n) is None, (shape, m, dist)


# ---- the slab fills: the selector on a shard of two or three targets, per slab ----------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "af", "peq"])
@SHAPES
def test_edges_and_components_over_small_slabs(ctx, native_built, shape, metric):
    """fill_edges and fill_components with slabs of two or three targets (each slab a fill of its own on a shard of those targets),
    at a threshold that occurs in the matrix -- its median element --: the edges from the oracle's vector under '<=' / '>=', the
    labels from the host statement under the strict and the non-strict predicate."""
    from phamclust_amd.hip import Context
    packed = WE.collection(shape)
    n = packed.n_genomes
    slab_bytes = 8 * 3 * (n - 1)                                         # targets n - 3 ... n - 1 have 3 n - 6 pairs: three to a slab, two never split
    cuts = Context.edge_slabs(n, slab_bytes)
    n_slabs = len(cuts) - 1
    top = [int(b - a) for a, b in zip(cuts[:-1], cuts[1:]) if a >= 3 * n // 4]                # (the first targets have few pairs: many to a slab)
    assert n_slabs >= 7 and max(top) == 3 and sum(k >= 2 for k in top) >= 2, cuts
    ctx.upload(packed, residues=metric == "peq")
    for dist in (True, False):
        dense = Dense(WE.oracle_fill(shape, metric, dist), n, dist)
        thr = median_value(dense.condensed)
        assert (dense.condensed == thr).any() and 0 < dense.passing(thr, True) < dense.passing(thr, False) <= packed.n_pairs
        want = expected_edges(dense.condensed, n, thr, dist)
        for sb, ns in ((slab_bytes, n_slabs), (0, 1)):
            *got, st = ctx.fill_edges(metric, thr, as_distance=dist, slab_bytes=sb, want_stats=True)
            assert_edges(got, want, (shape, metric, dist, thr, sb))
            assert st["n_edges"] == want[0].shape[0] == dense.passing(thr, False) and st["n_slabs"] == ns and st["n_pairs"] == packed.n_pairs
            for strict in (True, False):
                check(ctx, metric, dense, thr, strict, sb, ns, (shape, metric, dist, thr, strict, sb))
    assert ctx.shard_pairs() == packed.n_pairs


# ---- the walkers' domains on the numeric-edge genomes -------------------------------------------------------------------------------
EDGE_SUBSETS = pytest.mark.parametrize("subset", ["lo", "hi", "empty", "all"])


@EDGE_SUBSETS
def test_numeric_edges_rows_fill(ctx, native_built, subset):
    """fill_rows on genomes of 65,535 / 65,536 copies of a pham, 1,023 / 1,024 genes, entries of 65,535 / 65,536 residues and empty
    translations: all rows at once, then each row alone; every cell equals what the live reference wrote."""
    want = _edge_want(subset)
    packed = S.edge_packed(subset)
    n = packed.n_genomes
    ctx.upload(packed, residues=False)
    ctx.set_shard(0, 1)
    for m in SET_METRICS:
        for dist in (True, False):
            full = WE.square(want[(m, dist)], n, dist)
            assert np.array_equal(ctx.fill_rows(m, list(range(n)), dist), full), (subset, m, dist)
            for q in range(n):
                got = ctx.fill_rows(m, [q], dist)
                assert got.shape == (1, n) and np.array_equal(got[0], full[q]), (subset, m, dist, packed.names[q], got[0].tolist(), full[q].tolist())


@EDGE_SUBSETS
def test_numeric_edges_groups_fill(ctx, native_built, subset):
    """fill_groups on the same genomes: one group of everything, all two-member groups in one call, two overlapping groups."""
    want = _edge_want(subset)
    packed = S.edge_packed(subset)
    n = packed.n_genomes
    s, t = np.triu_indices(n, k=1)
    pairs = [[int(a), int(b)] for a, b in zip(s, t)]
    overlapping = [list(range(0, n - 1)), list(range(1, n))]
    ctx.upload(packed, residues=False)
    ctx.set_shard(0, 1)
    for m in SET_METRICS:
        for dist in (True, False):
            flat = want[(m, dist)]
            full = WE.square(flat, n, dist)
            assert np.array_equal(ctx.fill_groups(m, [list(range(n))], dist)[0], flat), (subset, m, dist)
            got = ctx.fill_groups(m, pairs, dist)
            assert [v.shape for v in got] == [(1,)] * len(pairs) and np.array_equal(np.concatenate(got), flat), (subset, m, dist, "pairs")
            for group, values in zip(overlapping, ctx.fill_groups(m, overlapping, dist)):
                assert np.array_equal(values, WE.condensed_of(full, group)), (subset, m, dist, "overlapping")


@EDGE_SUBSETS
def test_numeric_edges_slab_fills(ctx, native_built, subset):
    """fill_edges and fill_components on the same genomes with ONE target per slab (each slab's fill runs the selector on a shard of
    one target) and without slabs, at a threshold equal to a value of the matrix."""
    from phamclust_amd.hip import Context
    want = _edge_want(subset)
    packed = S.edge_packed(subset)
    n = packed.n_genomes
    cuts = Context.edge_slabs(n, 8)
    n_slabs = len(cuts) - 1
    assert n_slabs == n - 1 and all(b - a == 1 for a, b in zip(cuts[:-1], cuts[1:]) if a >= 2)       # (targets 0 and 1 hold one pair between them)
    ctx.upload(packed, residues=False)
    for m in SET_METRICS:
        for dist in (True, False):
            dense = Dense(want[(m, dist)], n, dist)
            thr = median_value(dense.condensed)
            assert (dense.condensed == thr).any()
            expect = expected_edges(dense.condensed, n, thr, dist)
            for sb, ns in ((8, n_slabs), (0, 1)):
                *got, st = ctx.fill_edges(m, thr, as_distance=dist, slab_bytes=sb, want_stats=True)
                assert_edges(got, expect, (subset, m, dist, thr, sb))
                assert st["n_slabs"] == ns and st["n_edges"] == expect[0].shape[0] > 0
                for strict in (True, False):
                    check(ctx, m, dense, thr, strict, sb, ns, (subset, m, dist, thr, strict, sb))
    assert ctx.shard_pairs() == packed.n_pairs


def test_numeric_edges_aligned_metrics_are_refused(ctx, native_built):
    """The collection holds empty translations in shared phams, which cannot be aligned (the reference fails on them too): the rows
    and the groups domain refuse aai / peq with the library's data status, as the whole fill does, and fill the set metrics
    correctly afterwards."""
    from phamclust_amd import hip
    want = _edge_want("empty")
    packed = S.edge_packed("empty")
    n = packed.n_genomes
    ctx.upload(packed)
    with pytest.raises(hip.HipLibraryError, match="status -5"):
        ctx.fill_rows("peq", list(range(n)))
    with pytest.raises(hip.HipLibraryError, match="status -5"):
        ctx.fill_groups("aai", [list(range(n))])
    assert np.array_equal(ctx.fill_rows("af", list(range(n))), WE.square(want[("af", True)], n, True))
    assert np.array_equal(ctx.fill_groups("af", [list(range(n))])[0], want[("af", True)])
