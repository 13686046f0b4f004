"""The bounded nearest fill on the GPU: pc_fill_edges_bars against pc_fill_edges and the numpy predicate over the same build's whole
fill, pc_nearest_of_pairs against ``SparseEdges.nearest``, and the route -- ``_bounded_peq_nearest`` on a context,
``neighbors_de_novo(bound=True)`` and ``--af-bound`` -- against the plain nearest fill, element for element and bit for bit, with the
candidate count held to the numpy rule (tests/nearest_bound_cases.py) exactly.  The injected-value cases of the bars pass run in a
child process on the test-hooks twin of the library (tests/nearest_bound_driver.py)."""

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import nearest_bound_cases as NB
from conftest import REPO

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "tests", "nearest_bound_driver.py")
_WHOLE = {}
I32P, F64P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
PC_ERR_ARG, PC_ERR_STATE, PC_ERR_LIMIT = -1, -3, -4


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def whole_square(ctx, key, n, metric, as_distance):
    """The whole fill of the uploaded collection as a locked square, once per (collection, metric, direction)."""
    key = (key, metric, bool(as_distance))
    if key not in _WHOLE:
        full = np.zeros((n, n))
        s, t = np.triu_indices(n, k=1)
        full[s, t] = full[t, s] = np.array(ctx.fill(metric, as_distance))
        np.fill_diagonal(full, 1.0 - as_distance)
        full.flags.writeable = False
        _WHOLE[key] = full
    return _WHOLE[key]


def disjoint(n):
    """n genomes that share no pham: a collection that only sets N."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        g.add(f"p{k}", "MKTAYIAKQRQISFVK")
        genomes.append(g)
    return pack_genomes(genomes)


def three_slabs(n):
    from phamclust_amd import hip
    slab_bytes = 8 * (n * (n - 1) // 2 // 3 + n)
    assert len(hip.Context.edge_slabs(n, slab_bytes)) - 1 == 3
    return slab_bytes


def same_edges(got, want, label):
    for g, w, what in zip(got[:3], want[:3], ("src", "tgt", "val")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (label, what, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), (label, what)


def same_lists(got, want, label):
    assert np.array_equal(np.asarray(got[0]), np.asarray(want[0])), (label, "nbr")
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64), np.ascontiguousarray(want[1]).view(np.uint64)), (label, "val")


# ---- pc_fill_edges_bars -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "af", "peq"])
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_equal_bars_give_fill_edges(ctx, small_packed, synth200_packed, name, metric):
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    ctx.upload(packed)
    for as_distance, threshold in ((True, 0.75), (False, 0.25)):
        for slab_bytes in (0, three_slabs(n)):
            want = ctx.fill_edges(metric, threshold, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
            got = ctx.fill_edges_bars(metric, np.full(n, threshold), as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
            same_edges(got, want, (name, metric, as_distance, slab_bytes))
            assert 0 < len(got[0]) < n * (n - 1) // 2
            assert got[3]["n_slabs"] == want[3]["n_slabs"] == (3 if slab_bytes else 1) and got[3]["n_edges"] == want[3]["n_edges"] == len(got[0])
            assert got[3]["n_pairs"] == n * (n - 1) // 2 and got[3]["n_alignments"] == want[3]["n_alignments"]
    want = ctx.fill_edges(metric, 0.75)
    same_edges(ctx.fill_edges_bars(metric, np.full(n, 0.75), borrow=True), want, (name, metric, "lent"))


@pytest.mark.parametrize("metric", ["jc", "af", "peq"])
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_random_bars_follow_the_predicate(ctx, small_packed, synth200_packed, name, metric):
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    ctx.upload(packed)
    rng = np.random.default_rng(17)
    for as_distance in (True, False):
        whole = whole_square(ctx, name, n, metric, as_distance)
        present = np.unique(whole[np.triu_indices(n, k=1)])
        for round_ in range(2):
            bars = rng.choice(present, n)                                # bars AT values the fill delivers: the compare is non-strict
            bars[rng.random(n) < 0.1] = np.inf
            bars[rng.random(n) < 0.3] = -np.inf
            want = NB.edges_under_bars(whole, bars, as_distance)
            for slab_bytes in (0, three_slabs(n)):
                got = ctx.fill_edges_bars(metric, bars, as_distance=as_distance, slab_bytes=slab_bytes)
                same_edges(got, want, (name, metric, as_distance, round_, slab_bytes))
            assert 0 < len(want[0]) < n * (n - 1) // 2


def test_infinite_bars_and_one_open_genome(ctx, synth200_packed):
    n = synth200_packed.n_genomes
    ctx.upload(synth200_packed)
    pairs = n * (n - 1) // 2
    for as_distance in (True, False):
        whole = whole_square(ctx, "synth200", n, "af", as_distance)
        everything, nothing = (np.inf, -np.inf) if as_distance else (-np.inf, np.inf)
        got = ctx.fill_edges_bars("af", np.full(n, everything), as_distance=as_distance)
        same_edges(got, NB.edges_under_bars(whole, np.full(n, everything), as_distance), ("everything", as_distance))
        assert len(got[0]) == pairs
        assert len(ctx.fill_edges_bars("af", np.full(n, nothing), as_distance=as_distance, slab_bytes=three_slabs(n))[0]) == 0
        for g in (0, 1, 77, n - 1):                                      # one genome's bar admits its whole row, every other bar nothing
            bars = np.full(n, nothing)
            bars[g] = everything
            for slab_bytes in (0, three_slabs(n)):
                src, tgt, val = ctx.fill_edges_bars("af", bars, as_distance=as_distance, slab_bytes=slab_bytes)
                others = np.concatenate([np.arange(g), np.arange(g + 1, n)])
                assert np.array_equal(src, np.minimum(others, g)) and np.array_equal(tgt, np.maximum(others, g)), (g, as_distance, slab_bytes)
                assert np.array_equal(val, whole[g, others])


def test_bars_on_one_and_two_genomes(ctx):
    ctx.upload(disjoint(1), residues=False)
    for bars in ([0.5], [np.inf], [-np.inf]):
        src, tgt, val, st = ctx.fill_edges_bars("jc", bars, want_stats=True)
        assert len(src) == len(tgt) == len(val) == 0 and st["n_edges"] == 0
    ctx.upload(disjoint(2), residues=False)                              # one pair, distance 1.0
    for bars, listed in (([1.0, 0.0], 1), ([0.0, 1.0], 1), ([0.5, 0.999999], 0), ([np.inf, -np.inf], 1), ([-np.inf, -np.inf], 0)):
        src, tgt, val = ctx.fill_edges_bars("jc", bars)
        assert len(src) == listed, bars
        if listed:
            assert (src[0], tgt[0], val[0]) == (0, 1, 1.0)
    for bars, listed in (([0.0, 0.5], 1), ([0.5, 0.5], 0)):              # similarity 0.0
        assert len(ctx.fill_edges_bars("jc", bars, as_distance=False)[0]) == listed, bars


def test_bars_refusals(ctx, small_packed):
    from phamclust_amd import hip
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    with pytest.raises(ValueError, match="bars"):
        ctx.fill_edges_bars("jc", np.zeros(n - 1))
    lib, h = ctx._lib, ctx._h
    bars = np.full(n, 0.5)
    bars[11] = np.nan

    def call(metric, bar_ptr, slab_bytes=0, outputs=True):
        cells = [I32P(ctypes.c_int32(1)), I32P(ctypes.c_int32(1)), F64P(ctypes.c_double(1.0))]
        ne, nsl = ctypes.c_int64(7), ctypes.c_int32(7)
        rc = lib.pc_fill_edges_bars(h, metric, 1, bar_ptr, slab_bytes, ctypes.byref(cells[0]), ctypes.byref(cells[1]),
                                    ctypes.byref(cells[2]) if outputs else None, ctypes.byref(ne), ctypes.byref(nsl), None)
        return rc, [bool(c) for c in cells[:2]] + [ne.value, nsl.value], lib.pc_last_error().decode()
    rc, out, message = call(1, bars.ctypes.data_as(F64P))
    assert rc == PC_ERR_ARG and out == [False, False, 0, 0] and "genome 11" in message and "NaN" in message
    rc, out, message = call(1, None)
    assert rc == PC_ERR_ARG and out == [False, False, 0, 0] and "bar" in message
    good = np.full(n, 0.5)
    assert call(7, good.ctypes.data_as(F64P))[0] == PC_ERR_ARG                           # bad metric
    assert call(1, good.ctypes.data_as(F64P), slab_bytes=-1)[0] == PC_ERR_ARG
    assert call(1, good.ctypes.data_as(F64P), outputs=False)[0] == PC_ERR_ARG            # a NULL out pointer
    try:
        ctx.set_shard(1, 2)
        with pytest.raises(hip.HipLibraryError, match="status -3"):
            ctx.fill_edges_bars("jc", good)
    finally:
        ctx.set_shard(0, 1)
    ctx.upload(small_packed, residues=False)
    assert call(5, good.ctypes.data_as(F64P))[0] == PC_ERR_STATE                          # peq without the residues
    same_edges(ctx.fill_edges_bars("jc", good), ctx.fill_edges("jc", 0.5), "after the refusals")
    fresh = hip.Context(ctx.device_id)
    try:
        cells = [I32P(), I32P(), F64P()]
        ne, nsl = ctypes.c_int64(0), ctypes.c_int32(0)
        assert fresh._lib.pc_fill_edges_bars(fresh._h, 1, 1, good.ctypes.data_as(F64P), 0, *(ctypes.byref(c) for c in cells), ctypes.byref(ne),
                                             ctypes.byref(nsl), None) == PC_ERR_STATE
    finally:
        fresh.close()


@pytest.mark.parametrize("case", ["bars_chunk_edges"])
def test_bars_on_injected_values(native_built, case):
    env = dict(os.environ, PHAMCLUST_NATIVE_VARIANT="hooks", PHAMCLUST_NO_TORCH="1")
    run = subprocess.run([sys.executable, DRIVER, case], env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, f"case '{case}' ended with status {run.returncode}:\n{run.stdout[-4000:]}"
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[:2] == ["ok", case] and int(last[2]) > 0, run.stdout[-4000:]


# ---- pc_nearest_of_pairs --------------------------------------------------------------------------------------------------------
RUNS = (0, 1, 63, 64, 65, 129)                                           # pairs that touch genomes 0 .. 5


def star_list(n, rng):
    """Genome j < 6 paired with the first RUNS[j] genomes from 10 on: runs of exactly those lengths; values on six millionths."""
    src = np.concatenate([np.full(r, j, dtype=np.int32) for j, r in enumerate(RUNS)])
    tgt = np.concatenate([np.arange(10, 10 + r, dtype=np.int32) for r in RUNS])
    assert tgt.max() < n
    return src, tgt, rng.integers(0, 6, src.shape[0]) / 1000000.0


def host_lists(n, src, tgt, val, k, as_distance):
    from phamclust_amd.matrix import SparseEdges
    lo, hi = np.minimum(src, tgt), np.maximum(src, tgt)
    order = np.lexsort((lo, hi))
    return SparseEdges([f"g{i}" for i in range(n)], lo[order], hi[order], np.asarray(val)[order], is_distance=as_distance).nearest(k)


def test_nearest_of_pairs_at_the_run_lengths(ctx):
    n = 200
    ctx.upload(disjoint(n), residues=False)
    rng = np.random.default_rng(5)
    src, tgt, val = star_list(n, rng)
    shuffle = rng.permutation(src.shape[0])
    flip = rng.random(src.shape[0]) < 0.5
    s2, t2, v2 = np.where(flip, tgt, src)[shuffle], np.where(flip, src, tgt)[shuffle], val[shuffle]
    for as_distance in (True, False):
        for k in (1, 2, 63, 64):
            want = host_lists(n, src, tgt, val, k, as_distance)
            assert want[2][:6].tolist() == list(RUNS) and want[0].shape == (n, k)
            for label, listing in (("sorted", (src, tgt, val)), ("shuffled", (s2, t2, v2))):
                got = ctx.nearest_of_pairs(*listing, k, as_distance=as_distance)
                same_lists(got, want, (label, as_distance, k))
                assert np.array_equal(got[2], want[2]) and got[2].dtype == np.int32
                assert (got[0][0] == -1).all() and np.isnan(got[1][0]).all()                 # the genome no pair touches
    # distinct values as well: random doubles, negatives included
    wide = rng.standard_normal(src.shape[0])
    for as_distance in (True, False):
        same_lists(ctx.nearest_of_pairs(s2, t2, wide[shuffle], 64, as_distance=as_distance), host_lists(n, src, tgt, wide, 64, as_distance), ("wide", as_distance))
    lent = ctx.nearest_of_pairs(src, tgt, val, 5, borrow=True)
    same_lists(lent, host_lists(n, src, tgt, val, 5, True), "lent")


def test_nearest_of_no_pair_and_one_pair(ctx):
    n = 70
    ctx.upload(disjoint(n), residues=False)
    for as_distance in (True, False):
        nbr, val, count = ctx.nearest_of_pairs([], [], [], 3, as_distance=as_distance)
        assert nbr.shape == val.shape == (n, 3) and (nbr == -1).all() and np.isnan(val).all() and not count.any()
        nbr, val, count = ctx.nearest_of_pairs([69], [4], [0.25], 64, as_distance=as_distance)
        want = host_lists(n, np.array([69]), np.array([4]), np.array([0.25]), 64, as_distance)
        same_lists((nbr, val), want, ("one pair", as_distance))
        assert count.sum() == 2 and nbr[4, 0] == 69 and nbr[69, 0] == 4 and val[4, 0] == val[69, 0] == 0.25 and (nbr[:, 1:] == -1).all()
    ctx.upload(disjoint(1), residues=False)
    nbr, val, count = ctx.nearest_of_pairs([], [], [], 3)
    assert nbr.shape == (1, 0) and count.tolist() == [0]


def test_nearest_of_the_whole_triangle_is_fill_nearest(ctx, small_packed):
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    s, t = np.triu_indices(n, k=1)
    for as_distance in (True, False):
        values = np.array(ctx.fill("peq", as_distance))
        for k in (1, 4, 22, 64):
            want = ctx.fill_nearest("peq", k, as_distance=as_distance)
            got = ctx.nearest_of_pairs(t, s, values, k, as_distance=as_distance)
            same_lists(got, want, (as_distance, k))
            assert (got[2] == n - 1).all()


def test_nearest_of_pairs_refusals(ctx, small_packed):
    from phamclust_amd import hip
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    lib, h = ctx._lib, ctx._h
    src, tgt, val = np.array([1, 2, 7, 3], dtype=np.int32), np.array([2, 7, 1, 9], dtype=np.int32), np.array([0.1, 0.2, 0.3, 0.4])
    before = (src.copy(), tgt.copy(), val.copy())

    def call(s, t, v, n_pairs, k, handle=h, outputs=True):
        marks = (ctypes.c_int32(1), ctypes.c_double(1.0), ctypes.c_int32(1))
        cells = [I32P(marks[0]), F64P(marks[1]), I32P(marks[2])]
        kk = ctypes.c_int32(7)
        ptr = lambda a, typ: None if a is None else a.ctypes.data_as(typ)
        rc = lib.pc_nearest_of_pairs(handle, ptr(s, I32P), ptr(t, I32P), ptr(v, F64P), n_pairs, 1, k, ctypes.byref(cells[0]), ctypes.byref(cells[1]),
                                     ctypes.byref(cells[2]) if outputs else None, ctypes.byref(kk))
        return rc, [bool(c) for c in (cells if outputs else cells[:2])] + [kk.value], lib.pc_last_error().decode()
    cleared = [False, False, False, 0]
    assert call(src, tgt, val, 4, 0)[:2] == (PC_ERR_ARG, cleared)                         # k < 1
    assert call(src, tgt, val, 4, -3)[:2] == (PC_ERR_ARG, cleared)
    rc, out, message = call(src, tgt, val, 4, 65)
    assert (rc, out) == (PC_ERR_LIMIT, cleared) and "PC_NEAREST_MAX_K" in message
    assert call(src, tgt, val, -1, 3)[:2] == (PC_ERR_ARG, cleared)                        # n_pairs < 0
    for missing in ((None, tgt, val), (src, None, val), (src, tgt, None)):                # a NULL with n_pairs > 0
        assert call(*missing, 4, 3)[:2] == (PC_ERR_ARG, cleared)
    rc, out, message = call(src, tgt, val, 2 ** 30 + 1, 3)                                # above 2^30: before an entry is read
    assert (rc, out) == (PC_ERR_LIMIT, cleared) and "2^30" in message
    rc, out, _ = call(src, tgt, val, 4, 3, outputs=False)                                 # a NULL out pointer
    assert rc == PC_ERR_ARG and out == [False, False, 0]
    for bad in (n, -1):                                                                   # an index outside [0, N): the message names the entry
        for which in (0, 1):
            arrays = [src.copy(), tgt.copy()]
            arrays[which][2] = bad
            rc, out, message = call(arrays[0], arrays[1], val, 4, 3)
            assert (rc, out) == (PC_ERR_ARG, cleared) and "entry 2" in message
    diagonal = tgt.copy()
    diagonal[3] = src[3]
    rc, out, message = call(src, diagonal, val, 4, 3)
    assert (rc, out) == (PC_ERR_ARG, cleared) and "entry 3" in message and "diagonal" in message
    assert all(np.array_equal(a, b) for a, b in zip((src, tgt, val), before))
    rc, out, _ = call(None, None, None, 0, 3)                                             # n_pairs == 0: PC_OK
    assert rc == 0 and out == [True, True, True, 3]
    with pytest.raises(ValueError):
        ctx.nearest_of_pairs([1, 2], [3], [0.5, 0.5], 3)
    with pytest.raises(ValueError):
        ctx.nearest_of_pairs([1, 2], [3, 4], [0.5], 3)
    fresh = hip.Context(ctx.device_id)
    try:
        assert call(src, tgt, val, 4, 3, handle=fresh._h)[:2] == (PC_ERR_STATE, cleared)
    finally:
        fresh.close()
    # after all the refusals the call works, sharded or not (the context gives N only), without the residues too
    want = host_lists(n, src, tgt, val, 3, True)
    same_lists(ctx.nearest_of_pairs(src, tgt, val, 3), want, "after the refusals")
    try:
        ctx.set_shard(1, 2)
        same_lists(ctx.nearest_of_pairs(src, tgt, val, 3), want, "sharded")
    finally:
        ctx.set_shard(0, 1)
    ctx.upload(small_packed, residues=False)
    same_lists(ctx.nearest_of_pairs(src, tgt, val, 3), want, "no residues")


# ---- the route ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_distance", [True, False], ids=["distance", "similarity"])
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_bounded_lists_equal_the_plain_fill(ctx, small_packed, synth200_packed, name, as_distance):
    from phamclust_amd.results.neighbors import _bounded_peq_nearest
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    ctx.upload(packed)
    af_sim = whole_square(ctx, name, n, "af", False)
    peq = whole_square(ctx, name, n, "peq", as_distance)
    for k in (1, 4, 16, 64):
        plain_nbr, plain_val, plain = ctx.fill_nearest("peq", k, as_distance=as_distance, want_stats=True)
        nbr, val, st = _bounded_peq_nearest(ctx, k, as_distance, 0)
        same_lists((nbr, val), (plain_nbr, plain_val), (name, as_distance, k))
        rule = NB.bounded_rule(af_sim, peq, k, as_distance)
        assert st["n_candidates"] == rule["n_candidates"], (name, as_distance, k)          # exactly: no tolerance
        assert st["n_seed_pairs"] == len(rule["seed"][0]) and st["fallback"] == int(rule["fallback"]) and st["k"] == min(k, n - 1)
        assert st["af_ms_total"] > 0.0 and len(st["step_s"]) == 6
        if name == "small" and k >= 16:
            assert st["fallback"] == 1
        if name == "synth200" and k <= 16:
            assert st["fallback"] == 0
        if name == "synth200" and k == 4:
            assert 0 < st["n_alignments"] < plain["n_alignments"], (st["n_alignments"], plain["n_alignments"])
    sliced = _bounded_peq_nearest(ctx, 4, as_distance, three_slabs(n))
    same_lists(sliced, ctx.fill_nearest("peq", 4, as_distance=as_distance), (name, as_distance, "three slabs"))
    assert sliced[2]["n_slabs"] == 3 or sliced[2]["fallback"]


def test_neighbors_de_novo_bound_with_a_genome_apart(small_genomes):
    """``neighbors_de_novo(bound=True)`` on the small fixture and on it plus a genome that shares no pham with anyone: its bar is the
    worst value, so every one of its pairs is a candidate, and its list is the index order."""
    from phamclust_amd import cli, matrix as M
    from phamclust_amd.genome import Genome
    apart = Genome("zz_apart")
    apart.add("a pham of its own", "MKTAYIAKQRQISFVKSHFSRQ")
    apart.add("another of its own", "MSTNPKPQRKTKRNT")
    peq = cli.METRICS["peq"]
    for genomes in (small_genomes, sorted(list(small_genomes) + [apart], key=lambda g: g.name)):
        n = len(genomes)
        for as_distance in (True, False):
            for k in (1, 4):
                plain = M.neighbors_de_novo(genomes, peq, k, as_distance=as_distance)
                plain_alignments = M.LAST_FILL["n_alignments"]
                fast = M.neighbors_de_novo(genomes, peq, k, as_distance=as_distance, bound=True)
                st = dict(M.LAST_FILL)
                assert fast.nodes == plain.nodes and fast.is_distance == plain.is_distance
                same_lists((fast.indices, fast.weights), (plain.indices, plain.weights), (n, as_distance, k))
                assert st["metric"] == "peq" and st["n_gpus"] == 1 and st["n_candidates"] >= st["n_seed_pairs"] > 0
                if n > len(small_genomes):
                    g = fast.nodes.index("zz_apart")
                    assert fast.indices[g].tolist() == list(range(k)) and (fast.weights[g] == (1.0 if as_distance else 0.0)).all()
                    assert st["n_candidates"] >= n - 1
                if not st["fallback"]:
                    assert st["n_alignments"] <= 2 * plain_alignments


def test_cli_af_bound_writes_the_plain_routes_bytes(tmp_path):
    from phamclust_amd.scripts.phamclust import main
    tsv = os.path.join(REPO, "tests", "golden", "small_input.tsv")

    def run(name, *extra):
        out = tmp_path / name
        main([tsv, str(out), "-t", "1", "-m", "peq", *extra])
        return out
    for k in ("3", "16"):                                                # (16: the fallback)
        plain = run("plain" + k, "--nearest", k) / "nearest_peq.tsv"
        fast = run("fast" + k, "--nearest", k, "--af-bound")
        assert (fast / "nearest_peq.tsv").read_bytes() == plain.read_bytes() and plain.read_bytes().count(b"\n") == 23 * int(k)
        assert sorted(p.name for p in fast.iterdir() if p.is_file()) == ["nearest_peq.tsv", "phamclust.log"]
        assert "--af-bound:" in (fast / "phamclust.log").read_text()
