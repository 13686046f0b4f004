"""The joint fill (pc_fill_joint / pc_fill_pairs_joint and their _dev forms / Context.fill_joint / fill_pairs_joint / matrices_de_novo /
pairs_joint_de_novo / --also) on the GPU (run with ``-m gpu``).

A joint fill delivers up to six metrics of every pair off ONE plan and ONE alignment pass.  Every array it writes must EQUAL the
single-metric fill's, bit for bit (the int64 views are compared, not the doubles), and the oracle's; an array that was not asked for
must not be touched; the plan, its chunks and its counters must be the peq fill's; and the work above it must write the plain routes'
bytes."""

import ctypes
import os

import numpy as np
import pytest

import planner_cases as pc
import word_edge_cases as WE
from conftest import ALL_METRICS, REPO, SET_METRICS, golden_file, read_adjacency_condensed, read_lower_triangle, synth200_file
from test_gpu_rows import oracle_square              # the oracle's squares, computed once per session for the modules that share them

pytestmark = pytest.mark.gpu
BLOCK = 256
COUNTERS = ("n_alignments", "n_distinct_alignments", "n_cells", "n_tasks", "n_align_launches", "n_chunks")
MASKS = (("aai",), ("peq",), ("af", "peq"), ("gcs", "aai"), ("jc", "pocp", "aai", "peq"))
_SINGLE = {}


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def bits(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.float64)).view(np.int64)


def same(got, want):
    """Bit equality of two float64 arrays."""
    got, want = bits(got), bits(want)
    return got.shape == want.shape and bool((got == want).all())


def single_fills(ctx, key, as_distance):
    """``ctx.fill`` of the six metrics of the uploaded collection, once per (collection, direction), read-only."""
    key = (key, bool(as_distance))
    if key not in _SINGLE:
        _SINGLE[key] = {metric: np.array(ctx.fill(metric, as_distance)) for metric in ALL_METRICS}
        for arr in _SINGLE[key].values():
            arr.flags.writeable = False
    return _SINGLE[key]


# ---- 1: equals the single fills, the oracle and the reference-written files -----------------------------------------------------
@pytest.mark.parametrize("as_distance", [True, False], ids=["distance", "similarity"])
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_joint_equals_the_single_fills_and_the_oracle(ctx, small_packed, synth200_packed, name, as_distance):
    packed = small_packed if name == "small" else synth200_packed
    ctx.upload(packed)
    got = ctx.fill_joint(ALL_METRICS, as_distance=as_distance)
    assert list(got) == ALL_METRICS
    single = single_fills(ctx, name, as_distance)
    s, t = np.triu_indices(packed.n_genomes, k=1)
    for metric in ALL_METRICS:
        assert got[metric].dtype == np.float64 and got[metric].shape == (packed.n_pairs,)
        assert same(got[metric], single[metric]), (name, metric, as_distance, "single fill")
        assert same(got[metric], oracle_square(name, packed, metric, as_distance)[s, t]), (name, metric, as_distance, "oracle")
    for metric in SET_METRICS:                                    # the files the reference itself wrote (tests/test_gpu_parity.py reads them)
        if name == "small" and as_distance:
            names, gold, _ = read_lower_triangle(golden_file(metric))
        elif name == "small":
            names = packed.names
            gold, _ = read_adjacency_condensed(golden_file(metric, "similarity"), packed.names)
        elif as_distance:
            names, gold, _ = read_lower_triangle(synth200_file(metric))
        else:
            continue                                              # (synth200 has distance files only)
        assert names == packed.names and same(got[metric], gold), (name, metric, as_distance, "golden")


# ---- 2: masks; what was not asked for is not touched ------------------------------------------------------------------------------
@pytest.mark.parametrize("wanted", MASKS, ids="+".join)
def test_masks_write_the_asked_arrays_and_nothing_else(ctx, small_packed, wanted):
    import torch
    ctx.upload(small_packed)
    n_pairs = small_packed.n_pairs
    device = f"cuda:{ctx.device_id}"
    stream = torch.cuda.current_stream().cuda_stream
    for as_distance in (True, False):
        single = single_fills(ctx, "small", as_distance)
        buffers = {metric: torch.full((n_pairs + 1,), float("nan"), dtype=torch.float64, device=device) for metric in ALL_METRICS}
        nan_bits = bits(buffers["gcs"].cpu().numpy())
        # every address is handed over, asked for or not: the mask alone decides what is written
        mask = sum(1 << ALL_METRICS.index(metric) for metric in wanted)
        out = (ctypes.c_void_p * 6)(*[buffers[metric].data_ptr() for metric in ALL_METRICS])
        torch.cuda.synchronize()
        assert ctx._lib.pc_fill_joint_dev(ctx._h, mask, int(as_distance), out, ctypes.c_void_p(stream), None) == 0
        torch.cuda.synchronize()
        for metric in ALL_METRICS:
            host = buffers[metric].cpu().numpy()
            if metric in wanted:
                assert same(host[:-1], single[metric]), (wanted, metric, as_distance)
                assert bits(host[-1:])[0] == nan_bits[0]                       # one past the end
            else:
                assert (bits(host) == nan_bits).all(), (wanted, metric, as_distance, "untouched")
        # ... and with NULL for what is not asked for, through the wrapper
        st = ctx.fill_joint_dev(wanted, as_distance, {metric: buffers[metric].data_ptr() for metric in wanted}, stream=stream)
        torch.cuda.synchronize()
        assert st["n_chunks"] == 1 and st["n_pairs"] == n_pairs
        for metric in wanted:
            assert same(buffers[metric].cpu().numpy()[:-1], single[metric])
        host = ctx.fill_joint(wanted, as_distance=as_distance)
        assert list(host) == list(wanted) and all(same(host[metric], single[metric]) for metric in wanted)


# ---- 3, 6: chunks, and one alignment pass ------------------------------------------------------------------------------------------
def test_joint_runs_one_alignment_pass(ctx, synth200_packed):
    ctx.upload(synth200_packed)
    _, peq = ctx.fill("peq", want_stats=True)
    peq_tasks = ctx.last_plan_tasks()
    got, st = ctx.fill_joint(ALL_METRICS, want_stats=True)
    for key in COUNTERS + ("n_pairs", "n_residue_bytes", "n_distinct_cells"):
        assert st[key] == peq[key], key
    assert st["n_alignments"] > st["n_distinct_alignments"] > 0 and st["n_chunks"] == 1 and st["n_align_launches"] > 0
    assert np.array_equal(ctx.last_plan_tasks(), peq_tasks)
    assert st["ms_total"] > 0 and st["ms_align"] > 0 and st["ms_reduce"] > 0


def test_chunked_joint_fill_gives_the_same_values(ctx, synth200_packed):
    ctx.upload(synth200_packed)
    single = single_fills(ctx, "synth200", True)
    _, whole = ctx.fill("peq", want_stats=True)
    try:
        ctx.set_plan_budget(whole["n_alignments"] * 56 // 4)
        _, peq = ctx.fill("peq", want_stats=True)
        peq_tasks = ctx.last_plan_tasks()
        got, st = ctx.fill_joint(ALL_METRICS, want_stats=True)
        joint_tasks = ctx.last_plan_tasks()
        some, st_some = ctx.fill_joint(("af", "aai"), want_stats=True)
    finally:
        ctx.set_plan_budget(0)
    assert st["n_chunks"] >= 3, st["n_chunks"]
    for key in ("n_chunks", "n_alignments", "n_distinct_alignments", "n_cells", "n_tasks", "n_align_launches"):
        assert st[key] == peq[key] == st_some[key], key
    assert np.array_equal(joint_tasks, peq_tasks) and joint_tasks.sum() == st["n_tasks"]
    for metric in ALL_METRICS:
        assert same(got[metric], single[metric]), metric
    assert same(some["af"], single["af"]) and same(some["aai"], single["aai"])


# ---- 4: tile and word edges ----------------------------------------------------------------------------------------------------------
# k_walk's tiles are 32 x 32 genomes and its bitmap words are staged 32 per chunk: N = 31, 32, 33, 65 over 32, 33 and 65 words
EDGE_SHAPES = ((31, 32, 64), (32, 33, 1), (33, 65, 1), (65, 32, 64), (65, 33, 1), (65, 65, 1))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=WE.shape_id)
def test_joint_at_the_tile_and_word_edges(ctx, native_built, shape):
    packed = WE.collection(shape)
    assert packed.n_genomes == shape[0] and packed.words_per_row == shape[1]
    ctx.upload(packed)
    n = packed.n_genomes
    s, t = np.triu_indices(n, k=1)
    perm = np.random.default_rng(sum(shape)).permutation(s.shape[0])
    for as_distance in (True, False):
        got = ctx.fill_joint(ALL_METRICS, as_distance=as_distance)
        listed = ctx.fill_pairs_joint(ALL_METRICS, s[perm], t[perm], as_distance=as_distance)
        for metric in ALL_METRICS:
            flat = np.array(ctx.fill(metric, as_distance))
            assert same(flat, WE.oracle_fill(shape, metric, as_distance)), (shape, metric, as_distance, "whole fill")
            bad = np.flatnonzero(bits(got[metric]) != bits(flat))
            assert not bad.size, (shape, metric, as_distance, int(s[bad[0]]), int(t[bad[0]]), got[metric][bad[0]], flat[bad[0]], len(bad))
            assert same(listed[metric], flat[perm]), (shape, metric, as_distance, "pair list")


def two_genomes_over(n_words):
    """Two genomes (and a third, for N = 1: its first alone) over exactly 64 (n_words - 1) + 1 phams: the word_edge_cases generators
    place their extra genomes at index 7 and cannot build fewer than 8.  Genome a holds the even phams, b the odd ones, both the
    marks around every 32-word chunk boundary and the last pham; a few paralogs; translations from a small pool."""
    from phamclust_amd.genome import Genome
    P = WE.n_phams(n_words, 1)
    mark = set(WE.marks(n_words, 1))
    rng = np.random.default_rng(n_words)
    pool = ["".join(WE.LETTERS[int(c)] for c in rng.integers(0, 20, size=int(rng.integers(1, 31)))) for _ in range(12)]
    a, b = Genome("g0"), Genome("g1")
    for p in range(P):
        for genome, mine in ((a, p % 2 == 0), (b, p % 2 == 1)):
            if mine or p in mark:
                for _ in range(3 if p % 11 == 0 else 1):
                    genome.add(f"p{p:05d}", pool[int(rng.integers(len(pool)))])
    return [a, b]


def test_joint_of_two_genomes_and_of_one(ctx, native_built):
    from oracle import oracle
    from phamclust_amd.pack import pack_genomes
    genomes = two_genomes_over(33)
    packed = pack_genomes(genomes)
    assert packed.n_genomes == 2 and packed.words_per_row == 33
    ctx.upload(packed)
    for as_distance in (True, False):
        got = ctx.fill_joint(ALL_METRICS, as_distance=as_distance)
        listed = ctx.fill_pairs_joint(ALL_METRICS, [0, 1, 1], [1, 0, 1], as_distance=as_distance)
        for metric in ALL_METRICS:
            flat = np.array(ctx.fill(metric, as_distance))
            assert flat.shape == (1,) and same(got[metric], flat) and same(flat, oracle.fill(packed, metric, as_distance)), (metric, as_distance)
            assert same(listed[metric][:1], flat) and listed[metric][2] == 1.0 - as_distance
            assert same(listed[metric][1:2], ctx.fill_pairs(metric, [1], [0], as_distance))
    assert 0.0 < got["peq"][0] < 1.0 and 0.0 < got["gcs"][0] < 1.0               # the pair shares the marks, and only them
    # N = 1: every array has length 0 and the call succeeds
    ctx.upload(pack_genomes(genomes[:1]))
    got, st = ctx.fill_joint(ALL_METRICS, want_stats=True)
    assert list(got) == ALL_METRICS and all(arr.shape == (0,) for arr in got.values())
    assert st["n_pairs"] == 0 and st["n_alignments"] == 0
    assert ctx.fill_pairs_joint(("aai",), [0], [0])["aai"].tolist() == [0.0]


# ---- 5: every launch class ------------------------------------------------------------------------------------------------------------
def test_joint_fill_over_every_launch_class(ctx):
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    C = hip.Context
    packed = pack_genomes(pc.build(pc.design(C)))
    ctx.upload(packed)
    for as_distance in (True, False):
        single = {}
        for metric in ALL_METRICS:
            single[metric], peq = ctx.fill(metric, as_distance, want_stats=True)          # (peq last: its plan is the one on record)
        peq_tasks = ctx.last_plan_tasks()
        got, st = ctx.fill_joint(ALL_METRICS, as_distance=as_distance, want_stats=True)
        tasks = ctx.last_plan_tasks()
        assert np.array_equal(tasks, peq_tasks), "class by class"
        assert tasks.sum() == st["n_tasks"] == peq["n_tasks"] > 0
        reached = [pc.class_name(C, int(k)) for k in np.flatnonzero(tasks)]
        assert any("strip-mined" in x for x in reached) and any("one wave" in x for x in reached) and any("two waves" in x for x in reached)
        for metric in ALL_METRICS:
            assert same(got[metric], single[metric]), (metric, as_distance)


# ---- 7: pair lists ----------------------------------------------------------------------------------------------------------------------
def test_joint_pair_lists(ctx, synth200_packed):
    from oracle import oracle
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    n = synth200_packed.n_genomes
    reverse_packed = pack_genomes(sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:n][::-1])
    assert reverse_packed.names == synth200_packed.names[::-1]
    ctx.upload(synth200_packed)
    rng = np.random.default_rng(7)
    s_all, t_all = np.triu_indices(n, k=1)
    for as_distance in (True, False):
        single = single_fills(ctx, "synth200", as_distance)
        # forward entries, reversed entries, repeats and the diagonal in ONE list, in an order of the caller's
        pick = rng.choice(s_all.shape[0], 2 * BLOCK + 40, replace=False)
        s, t = s_all[pick], t_all[pick]
        loops = rng.integers(0, n, 9)
        src = np.concatenate([s, t, loops, s[:50]])
        tgt = np.concatenate([t, s, loops, t[:50]])
        order = rng.permutation(src.shape[0])
        got, st = ctx.fill_pairs_joint(ALL_METRICS, src[order], tgt[order], as_distance=as_distance, want_stats=True)
        _, peq = ctx.fill_pairs("peq", src[order], tgt[order], as_distance, want_stats=True)
        for key in COUNTERS + ("n_pairs",):
            assert st[key] == peq[key], key
        assert st["n_pairs"] == 2 * s.shape[0] + 50 and st["n_chunks"] == 1
        for metric in ALL_METRICS:
            backward = oracle.pairs(reverse_packed, metric, n - 1 - t, n - 1 - s, as_distance)
            want = np.concatenate([single[metric][pick], backward, np.full(9, 1.0 - as_distance), single[metric][pick[:50]]])
            assert same(got[metric], want[order]), (metric, as_distance)
            assert same(got[metric], ctx.fill_pairs(metric, src[order], tgt[order], as_distance)), (metric, as_distance, "single")
        if as_distance:
            forward = single["aai"][pick]
            assert (np.asarray(oracle.pairs(reverse_packed, "aai", n - 1 - t, n - 1 - s, True)) != forward).any(), "the orientation must show"
        # the block seams
        for length in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1):
            pick = rng.choice(s_all.shape[0], length, replace=False)
            got = ctx.fill_pairs_joint(ALL_METRICS, s_all[pick], t_all[pick], as_distance=as_distance)
            for metric in ALL_METRICS:
                assert got[metric].shape == (length,) and same(got[metric], single[metric][pick]), (metric, as_distance, length)
    # a budget that cuts the list into ranges
    pick = rng.choice(s_all.shape[0], 5 * BLOCK + 77, replace=False)
    s, t = s_all[pick].copy(), t_all[pick].copy()
    flip = rng.random(s.shape[0]) < 0.3
    s[flip], t[flip] = t[flip], s[flip].copy()
    t[::97] = s[::97]
    one, st1 = ctx.fill_pairs_joint(ALL_METRICS, s, t, want_stats=True)
    try:
        ctx.set_plan_budget((st1["n_alignments"] * 56 + s.shape[0] * 8) // 4)
        cut, st = ctx.fill_pairs_joint(ALL_METRICS, s, t, want_stats=True)
        _, peq = ctx.fill_pairs("peq", s, t, want_stats=True)
    finally:
        ctx.set_plan_budget(0)
    assert st["n_chunks"] >= 3 and st1["n_chunks"] == 1
    for key in COUNTERS:
        assert st[key] == peq[key], key
    for metric in ALL_METRICS:
        assert same(cut[metric], one[metric]) and same(one[metric], ctx.fill_pairs(metric, s, t)), metric


def test_fill_pairs_joint_dev_leaves_the_vectors_in_hbm(ctx, small_packed):
    import torch
    ctx.upload(small_packed)
    src, tgt = np.array([0, 3, 9, 22, 4, 4, 1]), np.array([3, 9, 22, 0, 5, 4, 9])
    wanted = ("pocp", "af", "peq")
    device = f"cuda:{ctx.device_id}"
    buffers = {metric: torch.full((src.shape[0] + 1,), float("nan"), dtype=torch.float64, device=device) for metric in ALL_METRICS}
    nan_bits = bits(buffers["gcs"].cpu().numpy())
    mask = sum(1 << ALL_METRICS.index(metric) for metric in wanted)
    out = (ctypes.c_void_p * 6)(*[buffers[metric].data_ptr() for metric in ALL_METRICS])
    i32p = ctypes.POINTER(ctypes.c_int32)
    s32, t32 = src.astype(np.int32), tgt.astype(np.int32)
    torch.cuda.synchronize()
    assert ctx._lib.pc_fill_pairs_joint_dev(ctx._h, mask, 1, s32.ctypes.data_as(i32p), t32.ctypes.data_as(i32p), src.shape[0], out,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None) == 0
    torch.cuda.synchronize()
    for metric in ALL_METRICS:
        host = buffers[metric].cpu().numpy()
        if metric in wanted:
            assert same(host[:-1], ctx.fill_pairs(metric, src, tgt)) and bits(host[-1:])[0] == nan_bits[0], metric
        else:
            assert (bits(host) == nan_bits).all(), metric
    st = ctx.fill_pairs_joint_dev(wanted, True, src, tgt, {metric: buffers[metric].data_ptr() for metric in wanted})
    torch.cuda.synchronize()
    assert st["n_pairs"] == src.shape[0] - 1 and same(buffers["peq"].cpu().numpy()[:-1], ctx.fill_pairs("peq", src, tgt))


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, small_packed):
    from phamclust_amd import hip
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    ctx.upload(small_packed)
    n, n_pairs = small_packed.n_genomes, small_packed.n_pairs
    single = single_fills(ctx, "small", True)
    lib, h = ctx._lib, ctx._h
    i32p = ctypes.POINTER(ctypes.c_int32)
    arrays = [np.full(n_pairs, np.nan) for _ in range(6)]
    nan_bits = bits(arrays[0]).copy()
    src, tgt = np.array([1, 2, 7, 7], dtype=np.int32), np.array([2, 7, 1, 7], dtype=np.int32)
    s_p, t_p = src.ctypes.data_as(i32p), tgt.ctypes.data_as(i32p)
    AAI, PEQ, ALL = 1 << 4, 1 << 5, 0x3f

    def outs(missing=()):
        return (ctypes.c_void_p * 6)(*[None if m in missing else arrays[m].ctypes.data for m in range(6)])

    def refused(status, text, call, *args):
        """The call answers `status` with `text` in its message, writes nothing, and the context still fills correctly."""
        assert call(*args) == status, (call.__name__, args)
        assert text in lib.pc_last_error().decode(), lib.pc_last_error().decode()
        assert all((bits(arr) == nan_bits).all() for arr in arrays)

    def still_fine(c=ctx):
        got = c.fill_joint(("af", "aai", "peq"))
        assert all(same(got[metric], single[metric]) for metric in got)

    for whole, pairs in ((True, False), (False, True)):
        def call(mask, out, *rest):
            if whole:
                return lib.pc_fill_joint(h, mask, 1, out, None)
            return lib.pc_fill_pairs_joint(h, mask, 1, *(rest or (s_p, t_p, 4)), out, None)
        refused(-1, "empty", call, 0, outs())                                               # mask 0
        refused(-1, "aai_ppos", call, PEQ | 1 << 6, outs())                                 # a bit above 5
        refused(-1, "aai_ppos", call, 1 << 31, outs())
        refused(-1, "millisecond", call, 0xf, outs())                                       # neither aai nor peq
        refused(-1, "millisecond", call, 1 << 3, outs())
        refused(-1, "out[3] (af) is NULL", call, ALL, outs(missing=(3,)))                    # a requested array that is NULL
        refused(-1, "out[5] (peq) is NULL", call, PEQ, outs(missing=(0, 1, 2, 3, 4, 5)))
        refused(-1, "out is NULL", call, PEQ, None)
        still_fine()
        assert call(AAI, outs(missing=(0, 1, 2, 3, 5))) == 0                                # ... and NULL where nothing is asked for is fine
        if whole:
            assert same(arrays[4], single["aai"])
        else:
            assert same(arrays[4][:4], ctx.fill_pairs("aai", src, tgt)) and (bits(arrays[4][4:]) == nan_bits[4:]).all()
        arrays[4][:] = np.nan
    dev = (ctypes.c_void_p * 6)()
    assert lib.pc_fill_joint_dev(h, PEQ, 1, dev, None, None) == -1 and "out[5]" in lib.pc_last_error().decode()
    assert lib.pc_fill_pairs_joint_dev(h, PEQ, 1, s_p, t_p, 4, dev, None, None) == -1 and "out[5]" in lib.pc_last_error().decode()

    # the pair-list form's index checks: pc_fill_pairs'
    def listed(*values):
        arr = np.array(values, dtype=np.int32)
        return arr, arr.ctypes.data_as(i32p)
    for bad in ((1, 2, n, 3), (1, 2, -1, 3)):
        keep, bad_p = listed(*bad)
        refused(-1, "entry 2", lib.pc_fill_pairs_joint, h, ALL, 1, bad_p, t_p, 4, outs(), None)
        refused(-1, "entry 2", lib.pc_fill_pairs_joint, h, ALL, 1, s_p, bad_p, 4, outs(), None)
    refused(-1, "n_pairs", lib.pc_fill_pairs_joint, h, ALL, 1, s_p, t_p, -1, outs(), None)
    refused(-1, "NULL", lib.pc_fill_pairs_joint, h, ALL, 1, None, t_p, 4, outs(), None)
    refused(-1, "NULL", lib.pc_fill_pairs_joint, h, ALL, 1, s_p, None, 4, outs(), None)
    refused(-4, "2^31-1", lib.pc_fill_pairs_joint, h, ALL, 1, s_p, t_p, 2 ** 31, outs(), None)
    assert lib.pc_fill_pairs_joint(h, ALL, 1, s_p, t_p, 0, outs(), None) == 0 and all((bits(arr) == nan_bits).all() for arr in arrays)
    assert lib.pc_fill_pairs_joint(h, 0, 1, s_p, t_p, 0, outs(), None) == -1                # the set is checked before the empty list is accepted
    still_fine()
    # the wrapper refuses the same sets before the library sees them
    for bad in ((), ("gcs", "af"), ("peq", "peq"), ("aai_ppos", "peq"), ("peq", "nope")):
        with pytest.raises(ValueError):
            ctx.fill_joint(bad)
        with pytest.raises(ValueError):
            ctx.fill_pairs_joint(bad, [0], [1])

    # a sharded context: refused as pc_fill_dev refuses one, and the shard state stays
    try:
        ctx.set_shard(1, 2)
        refused(-3, "sharded", lib.pc_fill_joint, h, ALL, 1, outs(), None)
        refused(-3, "sharded", lib.pc_fill_joint_dev, h, ALL, 1, outs(), None, None)
        refused(-3, "sharded", lib.pc_fill_pairs_joint, h, ALL, 1, s_p, t_p, 4, outs(), None)
        refused(-3, "sharded", lib.pc_fill_pairs_joint, h, 0, 1, s_p, t_p, 0, outs(), None)     # the state comes first
        assert ctx.shard_pairs() < n_pairs
    finally:
        ctx.set_shard(0, 1)
    still_fine()

    # no residues: the peq fill's refusal; the set metrics go on
    ctx.upload(small_packed, residues=False)
    refused(-3, "need the residues", lib.pc_fill_joint, h, ALL, 1, outs(), None)
    refused(-3, "need the residues", lib.pc_fill_pairs_joint, h, ALL, 1, s_p, t_p, 4, outs(), None)
    assert same(np.array(ctx.fill("af")), single["af"])
    still_fine()                                                                            # (the wrapper sends the residues after)

    # before any upload
    fresh = hip.Context(ctx.device_id)
    try:
        refused(-3, "upload first", fresh._lib.pc_fill_joint, fresh._h, ALL, 1, outs(), None)
        refused(-3, "upload first", fresh._lib.pc_fill_pairs_joint, fresh._h, ALL, 1, s_p, t_p, 4, outs(), None)
        fresh.upload(small_packed)
        still_fine(fresh)
    finally:
        fresh.close()

    # an empty translation: the peq fill's refusal
    empty, other, third = Genome("e1"), Genome("e2"), Genome("e3")
    empty.add("p1", "")
    other.add("p1", "MK")
    third.add("p1", "MKV"); third.add("p2", "MA")
    ctx.upload(pack_genomes([empty, other, third]))
    refused(-5, "empty translation", lib.pc_fill_joint, h, ALL, 1, outs(), None)
    refused(-5, "empty translation", lib.pc_fill_pairs_joint, h, ALL, 1, listed(1)[1], listed(2)[1], 1, outs(), None)
    with pytest.raises(hip.HipLibraryError, match="status -5"):
        ctx.fill("peq")
    ctx.upload(small_packed)
    still_fine()


# ---- 9: matrices_de_novo, pairs_joint_de_novo ----------------------------------------------------------------------------------------
def counting_uploads(M):
    uploads = []
    original = M.get_context().upload
    M.get_context().upload = lambda *a, **k: (uploads.append(1), original(*a, **k))[1]
    return uploads


def test_matrices_de_novo_equals_matrix_de_novo(small_genomes):
    from phamclust_amd import cli, matrix as M
    names = [g.name for g in small_genomes]
    for as_distance in (True, False):
        want = {metric: M.matrix_de_novo(small_genomes, cli.METRICS[metric], 1, as_distance=as_distance) for metric in ALL_METRICS}
        for wanted in (ALL_METRICS, ["peq", "af"], ["aai"], ["jc", "af"]):
            uploads = counting_uploads(M)
            try:
                got = M.matrices_de_novo(small_genomes, [cli.METRICS[metric] for metric in wanted], 1, as_distance=as_distance)
            finally:
                del M.get_context().upload
            assert len(uploads) == 1 and list(got) == wanted
            joint = "aai" in wanted or "peq" in wanted
            assert M.LAST_FILL["fills"] == (1 if joint else len(wanted)) and M.LAST_FILL["metrics"] == tuple(wanted)
            assert M.LAST_FILL["n_genomes"] == len(names) and (M.LAST_FILL["n_alignments"] > 0) == joint
            for metric in wanted:
                assert isinstance(got[metric], M.SymMatrix) and got[metric].nodes == names and got[metric].is_distance == as_distance
                assert same(got[metric].to_ndarray(), want[metric].to_ndarray()), (metric, as_distance, wanted)


def test_pairs_joint_de_novo_equals_pairs_de_novo(small_genomes):
    from phamclust_amd import cli, matrix as M
    names = [g.name for g in small_genomes]
    n = len(names)
    rng = np.random.default_rng(1)
    idx = [(int(a), int(b)) for a, b in rng.integers(0, n, (60, 2))]
    idx += [idx[0], idx[1][::-1], (3, 3)]                                                    # a repeat, a reversed repeat, the diagonal
    listing = [(names[a], b) if k % 3 == 0 else (a, names[b]) if k % 3 == 1 else (names[a], names[b]) for k, (a, b) in enumerate(idx)]
    for as_distance in (True, False):
        want = {metric: M.pairs_de_novo(small_genomes, cli.METRICS[metric], listing, as_distance=as_distance) for metric in ALL_METRICS}
        for wanted in (ALL_METRICS, ["af", "peq"], ["gcs", "pocp"]):
            uploads = counting_uploads(M)
            try:
                got = M.pairs_joint_de_novo(small_genomes, [cli.METRICS[metric] for metric in wanted], listing, as_distance=as_distance)
            finally:
                del M.get_context().upload
            assert len(uploads) == 1 and list(got) == wanted
            assert M.LAST_FILL["fills"] == (1 if "peq" in wanted else len(wanted)) and M.LAST_FILL["listed"] == len(idx)
            for metric in wanted:
                assert same(got[metric], want[metric]), (metric, as_distance, wanted)
                assert got[metric][-1] == 1.0 - as_distance
        assert same(M.pairs_joint_de_novo(small_genomes, [cli.METRICS["aai"]], np.asarray(idx), as_distance=as_distance)["aai"], want["aai"])


# ---- 10: the command line ---------------------------------------------------------------------------------------------------------------
def files_under(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())


def square_cells(path):
    """A squareform file as (its node order, {(row, column): the cell's text})."""
    lines = path.read_text().splitlines()
    nodes = lines[0].split("\t")[1:]
    cells = {}
    for line in lines[1:]:
        fields = line.split("\t")
        assert len(fields) == len(nodes) + 1
        for node, text in zip(nodes, fields[1:]):
            cells[(fields[0], node)] = text
    assert [line.split("\t")[0] for line in lines[1:]] == nodes
    return nodes, cells


def test_cli_also_on_the_dense_route(tmp_path):
    from phamclust_amd.scripts.phamclust import main
    tsv = os.path.join(REPO, "tests", "golden", "small_input.tsv")

    def run(name, *extra):
        out = tmp_path / name
        main([tsv, str(out), "-t", "1", *extra])
        return out
    plain = run("plain", "-m", "peq")
    joint = run("joint", "-m", "peq", "--also", "af,aai")
    # every file of the plain run is there, byte for byte (the log apart); beside them the --also files and nothing else.  The heatmap
    # renderings are held by presence: plotly writes random element ids into every .svg / .html, so two straight runs of one command
    # differ there too (tests/test_gpu_rows.py, tests/test_gpu_groups.py make the same exception)
    plain_files = [f for f in files_under(plain) if f != "phamclust.log"]
    assert len(plain_files) > 10 and "pairwise_peq_similarities.tsv" in plain_files and "pairwise_peq_adjacency.tsv" in plain_files
    for name in plain_files:
        assert (joint / name).is_file(), name
        if not name.endswith((".svg", ".html")):
            assert (joint / name).read_bytes() == (plain / name).read_bytes(), name
    cache = next(p.name for p in joint.iterdir() if p.name.endswith(".tmp"))
    extra = sorted(set(files_under(joint)) - set(plain_files) - {"phamclust.log"})
    assert extra == sorted([f"{cache}/02_distmats/af_distance_matrix.tsv", f"{cache}/02_distmats/aai_distance_matrix.tsv",
                            "pairwise_af_similarities.tsv", "pairwise_aai_similarities.tsv"])
    log_text = (joint / "phamclust.log").read_text()
    assert "ONE alignment pass" in log_text and log_text.count("parity:") == 1
    order, _ = square_cells(joint / "pairwise_peq_similarities.tsv")
    for metric in ("af", "aai"):
        alone = run(metric, "-m", metric)
        assert (joint / cache / "02_distmats" / f"{metric}_distance_matrix.tsv").read_bytes() == \
            (alone / cache / "02_distmats" / f"{metric}_distance_matrix.tsv").read_bytes(), metric
        nodes, cells = square_cells(joint / f"pairwise_{metric}_similarities.tsv")
        alone_nodes, alone_cells = square_cells(alone / f"pairwise_{metric}_similarities.tsv")
        assert nodes == order and sorted(alone_nodes) == sorted(nodes) and cells == alone_cells, metric
    # a second run reads all three caches and writes the same files
    again = tmp_path / "joint"
    rendered = lambda name: name == "phamclust.log" or name.endswith((".svg", ".html"))      # noqa: E731
    before = {name: (again / name).read_bytes() for name in files_under(again) if not rendered(name)}
    listed = files_under(again)
    main([tsv, str(again), "-t", "1", "-m", "peq", "--also", "af,aai"])
    assert files_under(again) == listed
    assert {name: (again / name).read_bytes() for name in files_under(again) if not rendered(name)} == before
    assert (again / "phamclust.log").read_text().count("read cached") == 3


def test_cli_also_with_pairs(tmp_path):
    from phamclust_amd.scripts.phamclust import main
    tsv = os.path.join(REPO, "tests", "golden", "small_input.tsv")
    names = sorted({line.split("\t")[0] for line in open(tsv)})
    rng = np.random.default_rng(3)
    listing = tmp_path / "pairs.tsv"
    picks = [(names[int(a)], names[int(b)]) for a, b in rng.integers(0, len(names), (80, 2))]
    picks += [picks[0], picks[1][::-1], (names[2], names[2])]
    listing.write_text("".join(f"{a}\t{b}\n" for a, b in picks))

    def run(name, *extra):
        out = tmp_path / name
        main([tsv, str(out), "-t", "1", "--pairs", str(listing), *extra])
        return out
    joint = run("joint", "-m", "peq", "--also", "jc,af,aai")
    assert sorted(p.name for p in joint.iterdir() if p.is_file()) == sorted([f"pairwise_{m}_pairs.tsv" for m in ("peq", "jc", "af", "aai")] + ["phamclust.log"])
    assert "ONE alignment pass" in (joint / "phamclust.log").read_text()
    for metric in ("peq", "jc", "af", "aai"):
        alone = run(metric, "-m", metric)
        got = (joint / f"pairwise_{metric}_pairs.tsv").read_bytes()
        assert got == (alone / f"pairwise_{metric}_pairs.tsv").read_bytes() and got.count(b"\n") == len(picks), metric
