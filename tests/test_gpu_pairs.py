"""The pair-list fill (pc_fill_pairs / Context.fill_pairs / pairs_de_novo / SparseEdges.rescored / edges_de_novo(prefilter=True) /
--pairs / --prefilter) on the GPU (run with ``-m gpu``).

A pair-list fill must give every listed entry the value of ``METRICS[metric](genomes[src], genomes[tgt])``, oriented as written:
with src < tgt the whole fill's cell bit for bit, reversed the oracle's value over the reverse-packed collection, src == tgt the
diagonal -- in the caller's order, whatever the list's length, its duplicates and the chunking; its counters are summed over the
entries while one plan merges duplicate sequence pairs; and the work above it must reproduce the plain routes element for element."""

import ctypes
import os

import numpy as np
import pytest

import planner_cases as pc
import word_edge_cases as WE
from conftest import ALL_METRICS, REPO, SET_METRICS
from test_gpu_rows import oracle_square              # the oracle's squares, computed once per session for the modules that share them

pytestmark = pytest.mark.gpu
SEVEN = ALL_METRICS + ["aai_ppos"]
BLOCK = 256
_WHOLE = {}


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def whole_square(ctx, key, n, metric, as_distance):
    """The whole fill of the uploaded collection as a square (diagonal preset), once per (collection, metric, direction)."""
    key = (key, metric, bool(as_distance))
    if key not in _WHOLE:
        full = np.zeros((n, n))
        s, t = np.triu_indices(n, k=1)
        full[s, t] = full[t, s] = np.array(ctx.fill(metric, as_distance))
        np.fill_diagonal(full, 1.0 - as_distance)
        full.flags.writeable = False
        _WHOLE[key] = full
    return _WHOLE[key]


@pytest.mark.parametrize("metric", SEVEN)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_pairs_equal_the_whole_fill_and_the_oracle(ctx, small_packed, synth200_packed, name, metric):
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    assert ctx._lib.pc_pair_block() == BLOCK
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    rng = np.random.default_rng(n)
    s_all, t_all = np.triu_indices(n, k=1)
    for as_distance in (True, False):
        flat = np.array(ctx.fill(metric, as_distance))
        want = oracle_square(name, packed, metric, as_distance)
        perm = rng.permutation(s_all.shape[0])
        got, st = ctx.fill_pairs(metric, s_all[perm], t_all[perm], as_distance, want_stats=True)
        assert got.dtype == np.float64 and got.shape == perm.shape
        assert np.array_equal(got, flat[perm]), (name, metric, as_distance)
        assert np.array_equal(got, want[s_all[perm], t_all[perm]]), (name, metric, as_distance, "oracle")
        assert st["n_pairs"] == perm.shape[0] and st["n_chunks"] == 1
        for length in (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):                 # the block seams
            pick = rng.choice(perm.shape[0], length, replace=length > perm.shape[0])
            assert np.array_equal(ctx.fill_pairs(metric, s_all[pick], t_all[pick], as_distance), flat[pick]), (name, metric, as_distance, length)
        # every entry twice (side by side after the sort), and the diagonal among them
        pick = rng.choice(perm.shape[0], min(300, perm.shape[0]), replace=False)
        once, st1 = ctx.fill_pairs(metric, s_all[pick], t_all[pick], as_distance, want_stats=True)
        twice_s, twice_t = np.concatenate([s_all[pick], s_all[pick][::-1]]), np.concatenate([t_all[pick], t_all[pick][::-1]])
        twice, st2 = ctx.fill_pairs(metric, twice_s, twice_t, as_distance, want_stats=True)
        assert np.array_equal(once, flat[pick]) and np.array_equal(twice, np.concatenate([flat[pick], flat[pick][::-1]]))
        for key in ("n_pairs", "n_alignments", "n_cells", "n_residue_bytes"):
            assert st2[key] == 2 * st1[key], key
        assert st2["n_distinct_alignments"] == st1["n_distinct_alignments"] and st2["n_tasks"] == st1["n_tasks"]
        assert (st1["n_alignments"] > 0) == (metric not in SET_METRICS)
        loops = rng.integers(0, n, 7)
        mixed_s, mixed_t = np.concatenate([loops[:3], s_all[pick], loops[3:]]), np.concatenate([loops[:3], t_all[pick], loops[3:]])
        mixed, st3 = ctx.fill_pairs(metric, mixed_s, mixed_t, as_distance, want_stats=True)
        assert np.array_equal(mixed, want[mixed_s, mixed_t]) and (mixed[:3] == 1.0 - as_distance).all() and (mixed[-4:] == 1.0 - as_distance).all()
        assert st3["n_pairs"] == pick.shape[0] and st3["n_alignments"] == st1["n_alignments"]
        only_loops, st4 = ctx.fill_pairs(metric, loops, loops, as_distance, want_stats=True)
        assert (only_loops == 1.0 - as_distance).all() and st4["n_pairs"] == 0 and st4["n_alignments"] == 0


def test_entries_are_oriented_as_written(ctx, synth200_packed):
    """aai(s, t) != aai(t, s) for some pairs (the anchor rule, metrics.py:208-209).  The reversed entry (t, s) must give the value of
    the reversed call: the oracle's over the same genomes packed in reverse order, where the pair's roles are swapped
    (tests/test_gpu_groups.py::test_aai_keeps_the_whole_fills_orientation has the construction)."""
    from oracle import oracle
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    n = synth200_packed.n_genomes
    reverse_packed = pack_genomes(sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:n][::-1])
    assert reverse_packed.names == synth200_packed.names[::-1]
    ctx.upload(synth200_packed)
    members = np.arange(1, n, 3)
    i, j = np.triu_indices(len(members), k=1)
    s, t = members[i], members[j]
    for metric in ("aai", "peq", "aai_ppos"):
        forward = np.asarray(oracle.pairs(synth200_packed, metric, s, t, True))
        backward = np.asarray(oracle.pairs(reverse_packed, metric, n - 1 - t, n - 1 - s, True))
        asymmetric = np.flatnonzero(forward != backward)
        if metric == "aai":
            assert asymmetric.size > 0, "the collection must hold pairs on which the orientation shows"
        assert np.array_equal(ctx.fill_pairs(metric, s, t), forward), metric
        assert np.array_equal(ctx.fill_pairs(metric, t, s), backward), metric
        # both orientations of the same pairs in ONE list, interleaved: each entry its own value
        both_s, both_t = np.stack([s, t], axis=1).reshape(-1), np.stack([t, s], axis=1).reshape(-1)
        got, st = ctx.fill_pairs(metric, both_s, both_t, want_stats=True)
        assert np.array_equal(got[0::2], forward) and np.array_equal(got[1::2], backward), metric
        assert st["n_pairs"] == 2 * s.shape[0]
        if metric == "aai":
            assert (got[0::2][asymmetric] != got[1::2][asymmetric]).all()
    for metric in SET_METRICS:
        for as_distance in (True, False):
            assert np.array_equal(ctx.fill_pairs(metric, t, s, as_distance), ctx.fill_pairs(metric, s, t, as_distance)), metric


@pytest.mark.parametrize("shape", [(65, 33, 1), (65, 64, 64), (65, 65, 1), (65, 1, 64)], ids=WE.shape_id)
def test_pairs_at_the_bitmap_chunk_edges(ctx, native_built, shape):
    """k_walk_pairs keeps one bit per scanned word in a 32-bit mask, 32 words at a time: collections ON the chunk edges (one word;
    a chunk and one bit; two chunks exactly; two and one bit), all pairs as one list, seven metrics, both directions."""
    packed = WE.collection(shape)
    n = packed.n_genomes
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    s, t = np.triu_indices(n, k=1)
    perm = np.random.default_rng(sum(shape)).permutation(s.shape[0])
    for metric in SEVEN:
        for as_distance in (True, False):
            flat = np.array(ctx.fill(metric, as_distance))
            assert np.array_equal(flat, WE.oracle_fill(shape, metric, as_distance)), (shape, metric, as_distance, "whole fill")
            got = ctx.fill_pairs(metric, s[perm], t[perm], as_distance)
            bad = np.flatnonzero(got != flat[perm])
            assert not bad.size, (shape, metric, as_distance, int(s[perm][bad[0]]), int(t[perm][bad[0]]), got[bad[0]], flat[perm][bad[0]], len(bad))


def test_pairs_fill_over_every_launch_class(ctx):
    """The designed collection of tests/planner_cases.py: the pairs with s = t (mod 3) equal the whole fill's cells, and the plan
    behind them reaches the strip-mined, the one-wave and the two-wave launch classes."""
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    C = hip.Context
    packed = pack_genomes(pc.build(pc.design(C)))
    n = packed.n_genomes
    s, t = np.triu_indices(n, k=1)
    keep = (s % 3) == (t % 3)
    s, t = s[keep], t[keep]
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    for metric, as_distance in (("aai", True), ("peq", True), ("peq", False), ("aai_ppos", True)):
        whole = whole_square(ctx, "designed", n, metric, as_distance)
        got, st = ctx.fill_pairs(metric, s, t, as_distance, want_stats=True)
        assert np.array_equal(got, whole[s, t]), (metric, as_distance)
        tasks = ctx.last_plan_tasks()
        assert tasks.sum() == st["n_tasks"] > 0
        reached = [pc.class_name(C, int(k)) for k in np.flatnonzero(tasks)]
        assert any("strip-mined" in x for x in reached) and any("one wave" in x for x in reached) and any("two waves" in x for x in reached)


def test_chunked_pairs_fill_gives_the_same_values(ctx, synth200_packed):
    n = synth200_packed.n_genomes
    rng = np.random.default_rng(5)
    s_all, t_all = np.triu_indices(n, k=1)
    pick = rng.choice(s_all.shape[0], 5 * BLOCK + 77, replace=False)
    s, t = s_all[pick].copy(), t_all[pick].copy()
    flip = rng.random(s.shape[0]) < 0.3                          # some entries reversed, some on the diagonal
    s[flip], t[flip] = t[flip], s[flip].copy()
    t[::97] = s[::97]
    length = s.shape[0]
    n_blocks = -(-length // BLOCK)
    ctx.upload(synth200_packed)
    for metric in ("peq", "aai"):
        one, st1 = ctx.fill_pairs(metric, s, t, want_stats=True)
        assert st1["n_chunks"] == 1 and st1["n_pairs"] == int((s != t).sum())
        try:
            # a fifth of what the plan (56 bytes per alignment) and the slot arrays (8 bytes per slot) of the whole request take
            ctx.set_plan_budget((st1["n_alignments"] * 56 + length * 8) // 5)
            cut, st = ctx.fill_pairs(metric, s, t, want_stats=True)
            assert 1 < st["n_chunks"] <= n_blocks
            ctx.set_plan_budget(56)                                    # one block per chunk
            single, st_single = ctx.fill_pairs(metric, s, t, want_stats=True)
            assert st_single["n_chunks"] == n_blocks
            assert ctx.last_plan_tasks().sum() == st_single["n_tasks"] > 0
        finally:
            ctx.set_plan_budget(0)
        for other, st_other in ((cut, st), (single, st_single)):
            assert np.array_equal(other, one)
            for key in ("n_pairs", "n_alignments", "n_cells", "n_residue_bytes"):
                assert st_other[key] == st1[key], key
        assert np.array_equal(ctx.fill_pairs(metric, s, t), one)


def test_statuses(ctx, small_packed):
    from phamclust_amd import hip
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    ctx.set_tie_rule(5)
    whole_jc = whole_square(ctx, "small tie 5", n, "jc", True)
    whole_aai = whole_square(ctx, "small tie 5", n, "aai", True)
    lib, h = ctx._lib, ctx._h
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    src, tgt = np.array([1, 2, 7, 7], dtype=np.int32), np.array([2, 7, 1, 7], dtype=np.int32)
    out = np.full(5, -1.0)
    s_p, t_p, out_p = src.ctypes.data_as(i32p), tgt.ctypes.data_as(i32p), out.ctypes.data_as(f64p)

    def listed(*values):
        arr = np.array(values, dtype=np.int32)
        return arr, arr.ctypes.data_as(i32p)
    assert lib.pc_fill_pairs(h, 7, 1, s_p, t_p, 4, out_p, None) == -1                       # bad metric
    assert lib.pc_fill_pairs(h, -1, 1, s_p, t_p, 4, out_p, None) == -1
    assert lib.pc_fill_pairs(h, 1, 1, s_p, t_p, -1, out_p, None) == -1                      # negative n_pairs
    assert lib.pc_fill_pairs(h, 1, 1, None, t_p, 4, out_p, None) == -1                      # a NULL pointer with n_pairs > 0
    assert lib.pc_fill_pairs(h, 1, 1, s_p, None, 4, out_p, None) == -1
    assert lib.pc_fill_pairs(h, 1, 1, s_p, t_p, 4, None, None) == -1
    assert lib.pc_fill_pairs_dev(h, 1, 1, s_p, t_p, 4, None, None, None) == -1
    for bad in ((1, 2, n, 3), (1, 2, -1, 3)):                                               # an index outside [0, N): the message names the entry
        for which in (0, 1):
            args = (listed(*bad)[1], t_p) if which == 0 else (s_p, listed(*bad)[1])
            assert lib.pc_fill_pairs(h, 1, 1, *args, 4, out_p, None) == -1
            assert "entry 2" in lib.pc_last_error().decode()
    assert lib.pc_fill_pairs(h, 1, 1, s_p, t_p, 2 ** 31, out_p, None) == -4                 # PC_ERR_LIMIT, before an entry is read
    assert lib.pc_fill_pairs_dev(h, 1, 1, s_p, t_p, 2 ** 31, out_p, None, None) == -4
    assert (out == -1.0).all()
    assert lib.pc_fill_pairs(h, 1, 1, None, None, 0, None, None) == 0                       # n_pairs == 0: PC_OK, nothing written
    assert lib.pc_fill_pairs(h, 1, 1, s_p, t_p, 0, out_p, None) == 0 and (out == -1.0).all()
    assert ctx.fill_pairs("jc", [], []).shape == (0,)
    assert lib.pc_fill_pairs(h, 1, 1, s_p, t_p, 4, out_p, None) == 0
    assert np.array_equal(out[:4], whole_jc[src, tgt]) and out[3] == 0.0 and out[4] == -1.0
    with pytest.raises(ValueError):
        ctx.fill_pairs("jc", [1, 2], [3])
    ctx.fill("jc")
    ctx.fill_pairs("af", [0], [1])                                                          # no selector: the last WHOLE fill stays on record
    assert ctx.last_set_launch()[0]["metric"] == "jc"
    # a sharded context: refused, and the shard state stays
    try:
        ctx.set_shard(1, 2)
        pairs = ctx.shard_pairs()
        with pytest.raises(hip.HipLibraryError, match="status -3"):
            ctx.fill_pairs("jc", [0], [1])
        assert lib.pc_fill_pairs(h, 1, 1, None, None, 0, None, None) == -3                  # the state is checked before the empty list is accepted
        assert ctx.shard_pairs() == pairs < n * (n - 1) // 2
    finally:
        ctx.set_shard(0, 1)
    # after all the refusals: still filling correctly, tie rule untouched
    assert ctx.tie_rule() == 5
    assert np.array_equal(ctx.fill_pairs("aai", src, tgt), whole_aai[src, tgt])
    s_all, t_all = np.triu_indices(n, k=1)
    assert np.array_equal(np.array(ctx.fill("aai")), whole_aai[s_all, t_all]) and ctx.shard_pairs() == n * (n - 1) // 2
    ctx.set_tie_rule(0)
    # aai before the residues are on the device
    ctx.upload(small_packed, residues=False)
    out[:] = -1.0
    assert lib.pc_fill_pairs(h, 4, 1, s_p, t_p, 4, out_p, None) == -3 and (out == -1.0).all()
    assert lib.pc_fill_pairs(h, 1, 1, s_p, t_p, 4, out_p, None) == 0 and np.array_equal(out[:4], whole_jc[src, tgt])
    # before any upload
    fresh = hip.Context(ctx.device_id)
    try:
        assert fresh._lib.pc_fill_pairs(fresh._h, 1, 1, s_p, t_p, 4, out_p, None) == -3
    finally:
        fresh.close()


def test_an_empty_translation_is_refused_as_by_the_whole_fill(ctx, small_packed):
    from phamclust_amd import hip
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    empty, other, third = Genome("e1"), Genome("e2"), Genome("e3")
    empty.add("p1", "")
    other.add("p1", "MK")
    third.add("p1", "MKV"); third.add("p2", "MA")
    ctx.upload(pack_genomes([empty, other, third]))
    for metric in ("aai", "peq", "aai_ppos"):
        for listing in (([0], [1]), ([1], [2]), ([2, 1], [1, 2])):                          # checked collection-wide, as a whole fill
            with pytest.raises(hip.HipLibraryError, match="status -5"):
                ctx.fill_pairs(metric, *listing)
    for metric in ("af", "jc"):
        flat = np.array(ctx.fill(metric, as_distance=False))                                # pairs (0, 1), (0, 2), (1, 2)
        assert np.array_equal(ctx.fill_pairs(metric, [0, 2, 1], [1, 0, 2], as_distance=False), flat)
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    assert np.array_equal(ctx.fill_pairs("peq", [1, 7], [2, 9]), whole_square(ctx, "small", n, "peq", True)[[1, 7], [2, 9]])


def test_fill_pairs_dev_leaves_the_vector_in_hbm(ctx, small_packed):
    import torch
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    whole = whole_square(ctx, "small", n, "peq", True)
    src, tgt = np.array([0, 3, 9, 22, 4, 4, 1]), np.array([3, 9, 22, 0, 5, 4, 9])
    forward = src <= tgt
    out = torch.full((src.shape[0] + 1,), -1.0, dtype=torch.float64, device=f"cuda:{ctx.device_id}")
    st = ctx.fill_pairs_dev("peq", True, src, tgt, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert st["n_pairs"] == src.shape[0] - 1 and host[-1] == -1.0
    assert np.array_equal(host[:-1][forward], whole[src, tgt][forward])
    assert np.array_equal(host[:-1], ctx.fill_pairs("peq", src, tgt))


# ---- pairs_de_novo, SparseEdges.rescored, edges_de_novo(prefilter=True), the CLI ------------------------------------------
def test_pairs_de_novo_equals_the_matrix_cells(small_genomes):
    from phamclust_amd import cli, matrix as M
    names = [g.name for g in small_genomes]
    n = len(names)
    rng = np.random.default_rng(1)
    idx = [(int(a), int(b)) for a, b in rng.integers(0, n, (60, 2))]
    listing = [(names[a], b) if k % 3 == 0 else (a, names[b]) if k % 3 == 1 else (names[a], names[b]) for k, (a, b) in enumerate(idx)]
    for metric in ALL_METRICS:
        func = cli.METRICS[metric]
        for as_distance in (True, False):
            whole = M.matrix_de_novo(small_genomes, func, 1, as_distance=as_distance)
            uploads = []
            original = M.get_context().upload
            try:
                M.get_context().upload = lambda *a, **k: (uploads.append(1), original(*a, **k))[1]
                got = M.pairs_de_novo(small_genomes, func, listing, as_distance=as_distance)
            finally:
                del M.get_context().upload
            assert len(uploads) == 1 and got.dtype == np.float64 and got.shape == (len(idx),)
            for (a, b), value in zip(idx, got):
                if a <= b or metric in SET_METRICS:                  # (reversed aai / peq entries: test_entries_are_oriented_as_written)
                    assert value == whole.get_weight(names[a], names[b]), (metric, as_distance, a, b)
            assert np.array_equal(got, M.pairs_de_novo(small_genomes, func, np.asarray(idx), as_distance=as_distance))
    assert M.LAST_FILL["metric"] == "peq" and M.LAST_FILL["listed"] == len(idx)


def test_rescored_edges_carry_the_other_metrics_cells(small_genomes):
    from phamclust_amd import cli, matrix as M
    jc = M.edges_de_novo(small_genomes, cli.METRICS["jc"], 0.9)
    assert 0 < len(jc) < len(small_genomes) * (len(small_genomes) - 1) // 2
    for as_distance in (None, True, False):
        direction = True if as_distance is None else as_distance
        whole = M.matrix_de_novo(small_genomes, cli.METRICS["peq"], 1, as_distance=direction).to_ndarray()
        got = jc.rescored(small_genomes, cli.METRICS["peq"], as_distance=as_distance)
        assert got.nodes == jc.nodes and np.array_equal(got.source, jc.source) and np.array_equal(got.target, jc.target)
        assert got.threshold is None and got.is_distance == direction
        assert np.array_equal(got.weight, whole[jc.source, jc.target])


@pytest.mark.parametrize("name, threshold, as_distance", [("small", 0.75, True), ("small", 0.5, True), ("synth200", 0.75, True), ("synth200", 0.5, True),
                                                          ("synth200", 0.25, True), ("small", 0.25, False)])
def test_prefiltered_peq_edges_equal_the_plain_list(small_genomes, name, threshold, as_distance):
    from phamclust_amd import cli, matrix as M
    from phamclust_amd.synth import synth_genomes
    genomes = small_genomes if name == "small" else sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:200]
    plain = M.edges_de_novo(genomes, cli.METRICS["peq"], threshold, as_distance=as_distance)
    plain_alignments = M.LAST_FILL["n_alignments"]
    fast = M.edges_de_novo(genomes, cli.METRICS["peq"], threshold, as_distance=as_distance, prefilter=True)
    st = dict(M.LAST_FILL)
    assert fast.nodes == plain.nodes and fast.threshold == plain.threshold and fast.is_distance == plain.is_distance
    assert np.array_equal(fast.source, plain.source) and np.array_equal(fast.target, plain.target) and np.array_equal(fast.weight, plain.weight)
    assert st["n_edges"] == len(plain) <= st["n_candidates"] and st["n_alignments"] <= plain_alignments
    if (name, threshold) == ("synth200", 0.25):
        assert len(plain) == 0 and st["n_alignments"] == 0                      # no pair of the collection is that close: nothing is aligned
    elif (name, threshold) in (("small", 0.75), ("small", 0.25)):
        assert 0 < len(plain) < st["genome_pairs"]


def test_cli_pairs_and_prefilter_write_the_plain_routes_bytes(tmp_path):
    from phamclust_amd.scripts.phamclust import main
    tsv = os.path.join(REPO, "tests", "golden", "small_input.tsv")

    def run(name, *extra):
        out = tmp_path / name
        main([tsv, str(out), "-t", "1", *extra])
        return out
    plain = run("plain", "-m", "peq", "--adjacency-only", "--edge-thresh", "0.25") / "pairwise_peq_adjacency.tsv"
    fast = run("fast", "-m", "peq", "--adjacency-only", "--edge-thresh", "0.25", "--prefilter") / "pairwise_peq_adjacency.tsv"
    assert plain.read_bytes() == fast.read_bytes() and plain.read_bytes().count(b"\n") > 23
    # an adjacency file names its pairs in its first two columns: the peq file read back as a pair list gives its own bytes, ...
    again = run("again", "-m", "peq", "--pairs", str(plain))
    assert (again / "pairwise_peq_pairs.tsv").read_bytes() == plain.read_bytes()
    assert sorted(p.name for p in again.iterdir() if p.is_file()) == ["pairwise_peq_pairs.tsv", "phamclust.log"]
    # ... and the edges of a jc file, under peq, the peq file's values for those pairs
    jc = run("jc", "-m", "jc", "--adjacency-only", "--edge-thresh", "0.5") / "pairwise_jc_adjacency.tsv"
    everything = run("everything", "-m", "peq", "--adjacency-only") / "pairwise_peq_adjacency.tsv"
    value = {tuple(line.split("\t")[:2]): line for line in everything.read_text().splitlines()}
    rescored = (run("rescored", "-m", "peq", "--pairs", str(jc)) / "pairwise_peq_pairs.tsv").read_text().splitlines()
    listed = [tuple(line.split("\t")[:2]) for line in jc.read_text().splitlines()]
    assert [tuple(line.split("\t")[:2]) for line in rescored] == listed and len(listed) > 23
    for pair, line in zip(listed, rescored):
        assert line == value.get(pair, f"{pair[0]}\t{pair[1]}\t0.000000"), pair
