"""The nearest-neighbours fill (pc_fill_nearest / Context.fill_nearest / neighbors_de_novo / ``phamclust --nearest``) on the GPU.

Every expectation comes from a dense vector -- a golden file the live reference wrote, the oracle's fill, or the same context's whole
fill -- through ``NearestNeighbors.from_dense``, the host statement of the call's definition (held to the reference's
``nearest_neighbors`` in tests/test_nearest_host.py).  Every comparison is exact: ``np.array_equal`` on the indices and on the values.
"""

import ctypes
import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, golden_file, read_lower_triangle, synth200_file

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def expected(condensed, n, k, as_distance=True):
    """(indices, weights) the definition gives for a condensed vector."""
    from phamclust_amd.matrix import NearestNeighbors, SymMatrix
    if n < 2:
        return np.empty((n, 0), dtype=np.int32), np.empty((n, 0), dtype=np.float64)
    matrix = SymMatrix.from_condensed([f"n{g:05d}" for g in range(n)], np.asarray(condensed), is_distance=as_distance)
    found = NearestNeighbors.from_dense(matrix, k)
    return found.indices, found.weights


def check(ctx, metric, condensed, n, k, as_distance=True, slab_bytes=0, n_slabs=None, label=None):
    """One fill held to the dense vector: indices, values, kk, the pair count (and the slab count where the caller knows it)."""
    label = label or (metric, n, k, as_distance, slab_bytes)
    want_nbr, want_val = expected(condensed, n, k, as_distance)
    nbr, val, st = ctx.fill_nearest(metric, k, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
    kk = min(k, max(n - 1, 0))
    assert nbr.dtype == np.int32 and val.dtype == np.float64 and nbr.shape == val.shape == (n, kk), label
    assert np.array_equal(nbr, want_nbr), label
    assert np.array_equal(val, want_val), label
    assert st["k"] == kk and st["n_pairs"] == n * (n - 1) // 2 and st["ms_select"] >= 0.0 and st["ms_finish"] >= 0.0, label
    if n_slabs is not None:
        assert st["n_slabs"] == n_slabs, label
    return nbr, val, st


def hand_built(n, kind):
    """n genomes: "identical" -- the same 4 phams and translations everywhere (every value ties); "disjoint" -- no pham shared;
    "chain" -- genome g holds phams p{g} and p{g+1}, so only neighbours share one; "valley" -- genome g holds phams p0 .. p|g - n//2|:
    the middle genome holds one pham, the two ends the most, and genomes g and n - 1 - g are identical."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    text = "MKTAYIAKQRQISFVKSHFSRQ"
    genomes = []
    for g in range(n):
        one = Genome(f"g{g:04d}")
        if kind == "chain":
            one.add(f"p{g}", text)
            one.add(f"p{g + 1}", "MKTAYLAKQRQISWVKSHFARQ")
        elif kind == "valley":
            for j in range(abs(g - n // 2) + 1):
                one.add(f"p{j:03d}", text[: 8 + j % 12])
        else:
            for j in range(4):
                one.add(f"p{j}" if kind == "identical" else f"p{g}_{j}", text[: 12 + 3 * j])
        genomes.append(one)
    return pack_genomes(genomes)


_ORACLE = {}


def oracle_fill(name, packed, metric, as_distance):
    from oracle import oracle
    key = (name, metric, bool(as_distance))
    if key not in _ORACLE:
        _ORACLE[key] = np.asarray(oracle.fill(packed, metric, as_distance))
    return _ORACLE[key]


# ---- 1: the fixtures the live reference wrote ---------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_nearest_equals_the_dense_fixture(ctx, small_packed, synth200_packed, name, metric):
    from phamclust_amd.hip import Context
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    _, distances, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
    forced = 8 * 1000                                  # synth200: ranges of about five targets near the end; small: one range
    cut = Context.edge_slabs(n, forced)
    n_forced = len(cut) - 1
    assert n_forced == 1 if name == "small" else (n_forced >= 20 and cut[-1] - cut[-2] <= 6)
    ks = [1, 5, 16, 64] + ([n - 1] if n - 1 <= 64 else [])
    ctx.upload(packed)
    for as_distance in (True, False):
        condensed = distances if as_distance else oracle_fill(name, packed, metric, False)
        for k in ks:
            for slab_bytes, n_slabs in ((0, 1), (forced, n_forced)):
                check(ctx, metric, condensed, n, k, as_distance, slab_bytes, n_slabs, (name, metric, as_distance, k, slab_bytes))


# ---- 2: shapes where the kernels can go wrong ----------------------------------------------------------
SHAPES = [("identical", 65), ("identical", 130), ("disjoint", 65), ("disjoint", 130), ("chain", 65), ("chain", 130), ("valley", 129)]


@pytest.mark.parametrize("metric", ["jc", "peq"])
@pytest.mark.parametrize("kind,n", SHAPES)
def test_hand_built_shapes(ctx, kind, n, metric):
    """Collections of 65, 129 and 130 genomes -- one and two source blocks of 64 plus a ragged one, targets beyond a wave's 64 lanes --
    at k = 1, 63 and 64, in one slab, in three slabs (N = 130: [0, 89), [89, 126), [126, 130): a 64-boundary of sources inside each),
    and with 8-byte slabs: the first holds targets 0 and 1 (the cut never leaves target 0 alone when N > 1: it has no pair and always
    fits beside target 1), every other slab ONE target, so every list is merged N - 2 times through both passes.
    identical: every value ties, the index alone decides.  valley: for source 0 every target from the middle on improves on the last
    (the column pass inserts at every step), for every target the sources improve towards the middle (the row pass inserts), and
    genomes g and N - 1 - g are identical, so ties decide between them."""
    from phamclust_amd.hip import Context
    packed = hand_built(n, kind)
    ctx.upload(packed)
    dist = ctx.fill(metric)
    sim = ctx.fill(metric, as_distance=False)
    if kind == "identical":
        assert not dist.any() and (sim == 1.0).all()
    elif kind == "disjoint":
        assert (dist == 1.0).all() and not sim.any()
    elif kind == "valley" and metric == "jc":
        full = np.zeros((n, n))
        full[np.triu_indices(n, k=1)] = dist
        assert (np.diff(full[0, n // 2:]) < 0).all()                       # source 0: every target from the middle on is nearer
        for t in (1, n // 4, n // 2):
            assert (np.diff(full[:t, t]) < 0).all()                         # a target of the first half: every source is nearer than the last
        assert full[0, n - 1] == 0.0 and full[1, n - 2] == 0.0
    three = 8 * 4000
    if n == 130:
        assert Context.edge_slabs(n, three).tolist() == [0, 89, 126, 130]
    assert Context.edge_slabs(n, 8).tolist() == [0] + list(range(2, n + 1))
    for k in (1, 63, 64):
        for slab_bytes in (0, three) + ((8,) if k != 63 else ()):
            for as_distance, condensed in ((True, dist), (False, sim)):
                nbr, _, _ = check(ctx, metric, condensed, n, k, as_distance, slab_bytes, label=(kind, n, metric, k, as_distance, slab_bytes))
                if kind in ("identical", "disjoint"):
                    assert nbr.tolist() == [[h for h in range(n) if h != g][:k] for g in range(n)]


@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_fewer_genomes_than_k(ctx, metric):
    """Three genomes, k = 5: kk = 2; with 8-byte slabs two ranges, targets {0, 1} and {2}."""
    packed = hand_built(3, "chain")
    ctx.upload(packed)
    for as_distance in (True, False):
        condensed = ctx.fill(metric, as_distance=as_distance)
        for k in (1, 2, 5, 64):
            for slab_bytes, n_slabs in ((0, 1), (8, 2)):
                _, _, st = check(ctx, metric, condensed, 3, k, as_distance, slab_bytes, n_slabs)
                assert st["k"] == min(k, 2)
    ctx.upload(hand_built(2, "identical"))
    nbr, val, st = check(ctx, metric, ctx.fill(metric), 2, 3)
    assert nbr.tolist() == [[1], [0]] and val.tolist() == [[0.0], [0.0]] and st["k"] == 1


# ---- 3: mid size ------------------------------------------------------------------------------------------
_SYNTH = {}


def synth_packed(n):
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    if n not in _SYNTH:
        _SYNTH[n] = pack_genomes(sorted(synth_genomes(n, 5000), key=lambda g: g.name))
    return _SYNTH[n]


@pytest.mark.parametrize("metric", ["jc", "af"])
def test_mid_size_in_three_slabs(ctx, metric):
    """synth(2000, 5000): 31 source blocks and a ragged 32nd, targets of up to 1,999 sources, three slabs ([0, 1183), [1183, 1673),
    [1673, 2000)).  Afterwards the context is the unsharded one it was, and a loan ends with the next fill."""
    from phamclust_amd.hip import Context, HipLibraryError
    n, slab_bytes = 2000, 8 * 700000
    assert len(Context.edge_slabs(n, slab_bytes)) - 1 == 3
    ctx.upload(synth_packed(n), residues=False)
    dense = ctx.fill(metric)
    want_nbr, want_val = expected(dense, n, 16)
    nbr, val, st = ctx.fill_nearest(metric, 16, slab_bytes=slab_bytes, want_stats=True, borrow=True)
    assert np.array_equal(np.asarray(nbr), want_nbr) and np.array_equal(np.asarray(val), want_val)
    assert st["n_slabs"] == 3 and st["k"] == 16 and st["n_pairs"] == n * (n - 1) // 2 and st["ms_select"] > 0.0 and st["ms_finish"] > 0.0
    assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride()
    assert np.array_equal(ctx.fill(metric), dense)                         # unsharded again: the dense vector as before
    for lent in (nbr, val):
        with pytest.raises(HipLibraryError):                               # ... and that fill ended the loan
            np.asarray(lent)
    one_nbr, one_val = ctx.fill_nearest(metric, 16)                        # one slab, copies
    assert np.array_equal(one_nbr, want_nbr) and np.array_equal(one_val, want_val)
    assert isinstance(one_nbr, np.ndarray) and one_nbr.flags.writeable


# ---- 4: refusals and state ----------------------------------------------------------------------------------
def test_refusals_and_state(ctx, small_packed):
    from phamclust_amd.hip import HipLibraryError, _f64p, _i32p
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    _, distances, _ = read_lower_triangle(golden_file("jc"))
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_nearest("jc", 0)
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_nearest("jc", -4)
    with pytest.raises(HipLibraryError, match="status -4"):
        ctx.fill_nearest("jc", 65)
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_nearest("jc", 5, slab_bytes=-1)
    ctx.set_shard(1, 3)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):
            ctx.fill_nearest("jc", 5)
    finally:
        ctx.set_shard(0, 1)
    check(ctx, "jc", distances, n, 5, label="after the refusals")
    assert np.array_equal(ctx.fill("jc"), distances)
    ctx.upload(small_packed, residues=False)
    lib, h = ctx._lib, ctx._h

    def call(metric, k=5, nbr_out=True, slab_bytes=0):
        pn, pv, kk, ns = _i32p(), _f64p(), ctypes.c_int32(7), ctypes.c_int32(7)
        rc = lib.pc_fill_nearest(h, metric, 1, k, slab_bytes, ctypes.byref(pn) if nbr_out else None, ctypes.byref(pv), ctypes.byref(kk),
                                 ctypes.byref(ns), None)
        return rc, bool(pn), bool(pv), kk.value, ns.value

    assert call(5) == (-3, False, False, 0, 0)                    # peq before the residues
    assert call(4) == (-3, False, False, 0, 0) and call(6) == (-3, False, False, 0, 0)     # aai, aai with positives
    assert call(1, nbr_out=False) == (-1, False, False, 0, 0)
    assert call(9) == (-1, False, False, 0, 0) and call(-1) == (-1, False, False, 0, 0)
    assert call(1, k=0) == (-1, False, False, 0, 0)
    assert call(1, k=65) == (-4, False, False, 0, 0)
    assert call(1, slab_bytes=-8) == (-1, False, False, 0, 0)
    assert call(1) == (0, True, True, 5, 1)
    assert call(1, k=64) == (0, True, True, n - 1, 1)
    a, b = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.pc_last_nearest_times(h, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0      # no stats asked
    assert lib.pc_last_nearest_times(None, ctypes.byref(a), ctypes.byref(b)) == -1
    # one genome: kk = 0, nothing to list
    ctx.upload(hand_built(1, "identical"))
    for metric in ("jc", "peq"):
        nbr, val, st = ctx.fill_nearest(metric, 5, want_stats=True)
        assert nbr.shape == val.shape == (1, 0) and st["k"] == 0 and st["n_pairs"] == 0 and st["n_slabs"] == 0


def test_result_does_not_depend_on_the_cut(ctx, synth200_packed):
    ctx.upload(synth200_packed, residues=False)
    _, distances, _ = read_lower_triangle(synth200_file("jc"))
    first_nbr, first_val, _ = check(ctx, "jc", distances, 200, 16)
    for slab_bytes in (8, 8 * 300, 8 * 5000, 0):
        nbr, val = ctx.fill_nearest("jc", 16, slab_bytes=slab_bytes)
        assert np.array_equal(nbr, first_nbr) and np.array_equal(val, first_val), slab_bytes


# ---- 5: above the C-ABI ---------------------------------------------------------------------------------------
def test_nearest_run(tmp_path, small_genomes, native_built):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    from phamclust_amd.scripts.phamclust import main
    out = tmp_path / "out"
    main([os.path.join(GOLDEN, "small_input.tsv"), str(out), "-m", "jc", "--nearest", "5"])
    files = sorted(p.relative_to(out).as_posix() for p in out.rglob("*") if p.is_file() and "01_genomes" not in p.as_posix())
    assert files == ["nearest_jc.tsv", "phamclust.log"]                          # no matrix, no adjacency file, no clusters
    dense = M.matrix_de_novo(small_genomes, cli.METRICS["jc"], 1)                # the dense pipeline's matrix (distances)
    want = [f"{s}\t{t}\t{w:.6f}" for s, t, w in M.NearestNeighbors.from_dense(dense, 5).inverted()]
    assert len(want) == 23 * 5
    assert (out / "nearest_jc.tsv").read_text().splitlines() == want
    log = (out / "phamclust.log").read_text()
    assert "the 5 nearest of each of 23 genomes" in log and "slab(s)" in log and "done (--nearest: no clustering)" in log
    found = M.neighbors_de_novo(small_genomes, cli.METRICS["peq"], 64, as_distance=False, slab_bytes=8 * 40)
    assert found.k == 22 and not found.is_distance and M.LAST_FILL["n_slabs"] > 1 and M.LAST_FILL["metric"] == "peq" and M.LAST_FILL["k"] == 22
    sim = M.matrix_de_novo(small_genomes, cli.METRICS["peq"], 1, as_distance=False)
    want = M.NearestNeighbors.from_dense(sim, 22)
    assert np.array_equal(found.indices, want.indices) and np.array_equal(found.weights, want.weights) and found.nodes == want.nodes
