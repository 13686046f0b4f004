"""The rows form of the nearest-neighbours fill (pc_fill_rows_nearest, Context.fill_rows_nearest, neighbors_extend, --grow-nearest) on
the GPU (run with ``-m gpu``).

Stored k-nearest lists over a subset of the genomes are grown by the others.  The stored lists and the expected ones both come from a
DENSE vector -- a golden file the live reference wrote, or the same context's whole fill, which the rest of the suite pins -- through
``NearestNeighbors.from_dense``; tests/test_rows_nearest_host.py holds the ``extended`` statement to it.  Every assertion is exact:
``np.array_equal`` on indices and on the bits of values.  A diagonal taken for a candidate, a pair of two new genomes missed in one of
their rows, a candidate index that is the slab row instead of its genome, a seed dropped, re-indexed wrongly or kept for a new genome,
a column block or row tile carried wrongly over its seam, an orientation that follows the row instead of the order, or a tie resolved by
arrival order fails here."""

import ctypes

import numpy as np
import pytest

from conftest import ALL_METRICS, golden_file, read_lower_triangle, synth200_file

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def square_of(condensed, n, as_distance):
    full = np.zeros((n, n))
    full[np.triu_indices(n, k=1)] = np.asarray(condensed)
    full = full + full.T
    np.fill_diagonal(full, 0.0 if as_distance else 1.0)
    return full


class Dense:
    """A dense matrix over n genomes and what ``NearestNeighbors.from_dense`` says of it and of its blocks (computed once per key)."""

    def __init__(self, square, as_distance):
        self.square, self.as_distance, self.n = square, as_distance, square.shape[0]
        self.names = [f"n{k:05d}" for k in range(self.n)]
        self._memo = {}

    def nearest(self, at, k):
        from phamclust_amd.matrix import NearestNeighbors, _square_matrix
        key = (tuple(at), k)
        if key not in self._memo:
            at = np.asarray(at, dtype=np.int64)
            if at.shape[0] == 0:
                self._memo[key] = NearestNeighbors([], np.empty((0, 0)), np.empty((0, 0)), is_distance=self.as_distance)
            else:
                block = _square_matrix([self.names[g] for g in at.tolist()], self.square[np.ix_(at, at)].copy(), self.as_distance)
                self._memo[key] = NearestNeighbors.from_dense(block, k)
        return self._memo[key]

    def seed(self, new, k):
        """(old positions, the stored lists of the old block as ``[n, k_stored]`` seed arrays in the grown numbering, or None)."""
        taken = set(new)
        old = np.asarray([g for g in range(self.n) if g not in taken], dtype=np.int64)
        stored = self.nearest(old.tolist(), k)
        if old.shape[0] == 0 or stored.k == 0:
            return old, None
        nbr = np.full((self.n, stored.k), -7, dtype=np.int32)                 # (rows of new genomes are ignored: anything may stand there)
        val = np.full((self.n, stored.k), np.nan)
        nbr[old], val[old] = old[stored.indices], stored.weights
        return old, (nbr, val)


def grow(ctx, metric, dense, new, k, slab_bytes=0, label=None, want_slabs=None):
    """The rows form from the stored lists of the old block, held to ``from_dense`` of the whole matrix."""
    n = dense.n
    new = sorted(int(g) for g in new)
    label = (label, metric, dense.as_distance, tuple(new) if len(new) < 8 else len(new), k, slab_bytes)
    _, seed = dense.seed(new, k)
    want = dense.nearest(range(n), k)
    nbr, val, st = ctx.fill_rows_nearest(metric, k, new, seed=seed, as_distance=dense.as_distance, slab_bytes=slab_bytes, want_stats=True)
    assert nbr.dtype == np.int32 and val.dtype == np.float64 and nbr.shape == val.shape == (n, min(k, n - 1)), label
    assert np.array_equal(nbr, want.indices), label
    assert same_bits(val, want.weights), label
    assert st["k"] == min(k, n - 1), label
    if want_slabs is not None:
        assert st["n_slabs"] == want_slabs, label
    return st


def new_sets(n):
    """The new genomes: the first, the last, two adjacent middle ones, all but one, every second."""
    return {"first": [0], "last": [n - 1], "middle": [n // 2, n // 2 + 1], "one_old": [g for g in range(n) if g != 5], "second": list(range(1, n, 2))}


_GOLDEN = {}


def golden_dense(ctx, metric, as_distance):
    key = (metric, as_distance)
    if key not in _GOLDEN:
        if as_distance:
            _, values, _ = read_lower_triangle(golden_file(metric))
        else:
            values = ctx.fill(metric, as_distance=False)
        _GOLDEN[key] = Dense(square_of(values, ctx.n_genomes, as_distance), as_distance)
    return _GOLDEN[key]


# ---- 1: all six metrics on the 23 golden genomes ------------------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_golden_collection_grown_from_every_subset(ctx, small_packed, metric):
    """aai is not symmetric: a value oriented by its row instead of by the order fails.  jc and peq also as similarities."""
    ctx.upload(small_packed)
    n = small_packed.n_genomes
    for as_distance in ((True, False) if metric in ("jc", "peq") else (True,)):
        dense = golden_dense(ctx, metric, as_distance)
        for name, new in new_sets(n).items():
            for k in (1, 5, 22, 64):
                grow(ctx, metric, dense, new, k, label=name)


def test_the_golden_inputs_are_not_vacuous(ctx, small_packed):
    """Asserted from the dense expectation alone.  jc distances of the 23 golden genomes, the two adjacent middle genomes (11, 12)
    new, K = 5: of the 21 old genomes 14 lists change and 7 do not, and in the lists of genomes 1, 3, 5, 7, 9, 10 and 15 a new genome
    enters at an interior position (neither first nor last)."""
    ctx.upload(small_packed)
    n, k = small_packed.n_genomes, 5
    dense = golden_dense(ctx, "jc", True)
    new = new_sets(n)["middle"]
    old = np.asarray([g for g in range(n) if g not in new])
    stored, grown = dense.nearest(old.tolist(), k), dense.nearest(range(n), k)
    changed = [g for i, g in enumerate(old.tolist()) if not np.array_equal(old[stored.indices[i]], grown.indices[g])]
    assert changed and len(changed) < len(old), "every old list changes, or none does"
    interior = [g for g in changed if np.isin(grown.indices[g][1:k - 1], new).any()]
    assert interior, "no new genome enters an old list at an interior position"
    grow(ctx, "jc", dense, new, k, label="not vacuous")


# ---- 2: synth200, the slab cut ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "pocp", "peq"])
def test_synth200_under_every_slab_cut(ctx, synth200_packed, metric):
    from phamclust_amd.hip import Context
    ctx.upload(synth200_packed)
    n = synth200_packed.n_genomes
    _, values, _ = read_lower_triangle(synth200_file(metric))
    dense = Dense(square_of(values, n, True), True)
    new = [3, 4, 60, 97, 131, 198, 199]
    for slab_bytes, want in ((8 * n, 7), (8 * n * 2, 4), (8 * n * 3, 3), (0, 1)):
        if slab_bytes:
            assert Context.rows_slabs(n, len(new), slab_bytes) == want
        grow(ctx, metric, dense, new, 16, slab_bytes=slab_bytes, want_slabs=want, label="synth200")


# ---- 3: tile and block seams --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_tile_and_block_seams(ctx, n):
    """n genomes against the column pass's tile edge T (columns per workgroup, rows per tile): one column block that is short, full,
    or followed by a block of one column, and three blocks; m new rows one below, at, one above and two tiles above T, whole and cut
    into two slabs (so that two new genomes lie in different slabs and must still list each other).  n = 65 once more as
    similarities.  m = n: nothing stored, no seed -- fill_nearest's expectation."""
    from phamclust_amd.hip import Context
    from phamclust_amd.synth import synth_packed
    T = Context.nearest_rows_tile()
    assert T == 64
    ctx.upload(synth_packed(n, 300, seed=n), residues=False)
    forms = [Dense(square_of(ctx.fill("jc"), n, True), True)]
    if n == 65:
        forms.append(Dense(square_of(ctx.fill("jc", as_distance=False), n, False), False))
    counts = sorted({min(m, n) for m in (1, T - 1, T, T + 1, min(2 * T + 1, n), n)})
    for dense in forms:
        for m in counts:
            new = sorted(np.random.default_rng(m).choice(n, size=m, replace=False).tolist()) if m < n else list(range(n))
            for k in (1, 16, 64):
                if m == n:
                    assert dense.seed(new, k)[1] is None
                grow(ctx, "jc", dense, new, k, label=("seam", n, m), want_slabs=1)
                half = (m + 1) // 2
                grow(ctx, "jc", dense, new, k, slab_bytes=8 * n * half, label=("seam, two slabs", n, m), want_slabs=2 if m > 1 else 1)


# ---- 4: ties ------------------------------------------------------------------------------------------------------
def hand_built(n, twins=()):
    """n genomes of a chain -- genome k holds phams p{k} and p{k+1}, so only neighbours share one, all the same way -- or, with
    ``twins`` = "all", n identical genomes; else one more genome per entry of ``twins``, identical to that genome of the chain."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        if twins == "all":
            for j in range(4):
                g.add(f"p{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        else:
            g.add(f"p{k}", "MKTAYIAKQRQISFVKSHFSRQ")
            g.add(f"p{k + 1}", "MKTAYLAKQRQISWVKSHFARQ")
        genomes.append(g)
    if twins != "all":
        for i, k in enumerate(twins):
            g = Genome(f"g{n + i:04d}")
            g.add(f"p{k}", "MKTAYIAKQRQISFVKSHFSRQ")
            g.add(f"p{k + 1}", "MKTAYLAKQRQISWVKSHFARQ")
            genomes.append(g)
    return pack_genomes(genomes)


def test_identical_genomes_every_list_is_decided_by_index(ctx):
    """68 identical genomes: every value ties, so genome g lists the K smallest indices other than g -- wherever its candidates came from."""
    n = 68
    ctx.upload(hand_built(n, "all"))
    for metric in ("jc", "peq"):
        dense = Dense(square_of(ctx.fill(metric), n, True), True)
        assert (dense.square == 0.0).all()
        for k in (5, 64):
            want = dense.nearest(range(n), k)
            for g in (0, 3, 67):
                assert want.indices[g].tolist() == [h for h in range(n) if h != g][:k]
            for new in ([0, 30, 67], [1, 2, 3]):
                grow(ctx, metric, dense, new, k, label="identical")
                grow(ctx, metric, dense, new, k, slab_bytes=8 * n, label="identical, a row per slab", want_slabs=3)


def test_a_new_genome_identical_to_an_old_one(ctx):
    """A chain of 40 and two more genomes, twins of genomes 7 and 21 of the chain: each twin ties with its original in every list, so
    the index decides which of them comes first -- whether the original was stored and the twin arrives, or the other way round."""
    n = 42
    ctx.upload(hand_built(40, twins=(7, 21)))
    for metric in ("jc", "peq"):
        dense = Dense(square_of(ctx.fill(metric), n, True), True)
        assert dense.square[7, 40] == 0.0 and dense.square[21, 41] == 0.0 and np.array_equal(dense.square[7, :7], dense.square[40, :7])
        for new in ([40, 41], [7, 41], [7, 21], [6, 7, 8, 40]):
            for k in (3, 16):
                grow(ctx, metric, dense, new, k, label="twins")
                grow(ctx, metric, dense, new, k, slab_bytes=8 * n, label="twins, a row per slab", want_slabs=len(new))


# ---- 5: short stored lists, the seed's domain ---------------------------------------------------------------------
@pytest.mark.parametrize("n_old", [1, 2, 3])
def test_short_stored_lists(ctx, n_old):
    """N_old - 1 < K: the stored lists hold 0, 1 or 2 entries, the columns behind them begin as the sentinel and are filled by the
    new genomes alone."""
    from phamclust_amd.synth import synth_packed
    n, k = n_old + 10, 8
    ctx.upload(synth_packed(n, 300, seed=40 + n_old), residues=False)
    dense = Dense(square_of(ctx.fill("jc"), n, True), True)
    old = {1: [4], 2: [0, 7], 3: [2, 3, 12]}[n_old]
    new = [g for g in range(n) if g not in old]
    _, seed = dense.seed(new, k)
    assert (seed is None) == (n_old == 1) and (seed is None or seed[0].shape == (n, n_old - 1))
    grow(ctx, "jc", dense, new, k, label="short")
    grow(ctx, "jc", dense, new, k, slab_bytes=8 * n * 4, label="short, three slabs", want_slabs=3)


def raw_call(ctx, metric_id, k, rows, seed, k_seed=None):
    """pc_fill_rows_nearest as the C-ABI has it: (rc, nbr is NULL, val is NULL, k_out, n_slabs) with the outputs set to junk first."""
    from phamclust_amd import hip
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    junk_i, junk_d = (ctypes.c_int32 * 1)(1), (ctypes.c_double * 1)(1.0)
    pn, pv = ctypes.cast(junk_i, i32p), ctypes.cast(junk_d, f64p)
    kk, nsl = ctypes.c_int32(5), ctypes.c_int32(5)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    s_nbr = s_val = None
    if seed is not None:
        s_nbr, s_val = np.ascontiguousarray(seed[0], dtype=np.int32), np.ascontiguousarray(seed[1], dtype=np.float64)
        k_seed = s_nbr.shape[1] if k_seed is None else k_seed
    rc = hip.load().pc_fill_rows_nearest(ctx._h, metric_id, 1, k, rows.ctypes.data_as(i32p), rows.shape[0],
                                         s_nbr.ctypes.data_as(i32p) if s_nbr is not None else None,
                                         s_val.ctypes.data_as(f64p) if s_val is not None else None, int(k_seed or 0), 0,
                                         ctypes.byref(pn), ctypes.byref(pv), ctypes.byref(kk), ctypes.byref(nsl), None)
    return rc, not pn, not pv, kk.value, nsl.value, hip.load().pc_last_error().decode()


def test_seed_domain_and_no_rows(ctx, small_packed):
    from phamclust_amd import hip
    from phamclust_amd.hip import HipLibraryError
    ctx.upload(small_packed)
    n, k = small_packed.n_genomes, 5
    jc = hip.METRIC_IDS["jc"]
    dense = golden_dense(ctx, "jc", True)
    whole = dense.nearest(range(n), k)
    # n_rows == 0: the seed re-laid to kk columns
    wider = dense.nearest(range(n), 8)
    nbr, val, st = ctx.fill_rows_nearest("jc", k, [], seed=(wider.indices, wider.weights), want_stats=True)
    assert np.array_equal(nbr, whole.indices) and same_bits(val, whole.weights) and st["n_slabs"] == 0 and st["k"] == k
    # n_rows == N: no seed, fill_nearest's expectation; a seed given all the same is ignored
    nbr, val = ctx.fill_rows_nearest("jc", k, list(range(n)))
    assert np.array_equal(nbr, whole.indices) and same_bits(val, whole.weights)
    new = [3, 12]
    old, (s_nbr, s_val) = dense.seed(new, k)
    g, h = int(old[4]), int(old[9])
    refusals = []

    def tampered(edit):
        a, b = s_nbr.copy(), s_val.copy()
        edit(a, b)
        return a, b

    def swap(a, b):                                                          # a row that descends: two entries of distinct values exchanged
        j = next(j for j in range(k - 1) if b[g, j] != b[g, j + 1])
        a[g, [j, j + 1]], b[g, [j, j + 1]] = a[g, [j + 1, j]], b[g, [j + 1, j]]

    def tie_descends(a, b):                                                  # equal values, the larger index first
        b[h, 1] = b[h, 0]
        a[h, 0], a[h, 1] = max(a[h, 0], a[h, 1]), min(a[h, 0], a[h, 1])

    refusals.append(("below min", (s_nbr[:, :k - 1], s_val[:, :k - 1]), "k_seed 4 is below"))
    refusals.append(("no seed", None, "a seed array is NULL"))                 # (NULL arrays with k_seed = 5; Python's seed=None says k_seed = 0)
    refusals.append(("beyond N", tampered(lambda a, b: a.__setitem__((g, 2), n)), "is no other old genome"))
    refusals.append(("negative", tampered(lambda a, b: a.__setitem__((g, 0), -1)), "is no other old genome"))
    refusals.append(("a query genome", tampered(lambda a, b: a.__setitem__((g, k - 1), 12)), "is no other old genome"))
    refusals.append(("itself", tampered(lambda a, b: a.__setitem__((g, 1), g)), "is no other old genome"))
    refusals.append(("descends", tampered(swap), "does not come after the entry before it"))
    refusals.append(("tie descends", tampered(tie_descends), "does not come after the entry before it"))
    for what, seed, text in refusals:
        rc, no_nbr, no_val, kk, nsl, err = raw_call(ctx, jc, k, new, seed, k_seed=k if seed is None else None)
        assert rc == -1 and no_nbr and no_val and kk == 0 and nsl == 0 and text in err, (what, rc, err)     # PC_ERR_ARG, outputs nulled
        with pytest.raises(HipLibraryError, match="k_seed 0 is below" if seed is None else text):
            ctx.fill_rows_nearest("jc", k, new, seed=seed)
        grow(ctx, "jc", dense, new, k, label=("after the refusal", what))     # the context is usable: the next call succeeds
    with pytest.raises(HipLibraryError, match="strictly ascending"):
        ctx.fill_rows_nearest("jc", k, [4, 4], seed=(s_nbr, s_val))
    with pytest.raises(HipLibraryError, match="PC_NEAREST_MAX_K"):
        ctx.fill_rows_nearest("jc", 65, new, seed=(s_nbr, s_val))
    with pytest.raises(ValueError, match="seed must be two"):
        ctx.fill_rows_nearest("jc", k, new, seed=(s_nbr[:-1], s_val[:-1]))
    # a longer stored list is cut; the times of the call are reported
    _, longer = dense.seed(new, 9)
    nbr, val, st = ctx.fill_rows_nearest("jc", k, new, seed=longer, want_stats=True)
    assert np.array_equal(nbr, whole.indices) and same_bits(val, whole.weights)
    assert st["ms_select"] > 0.0 and st["ms_finish"] > 0.0 and st["n_pairs"] == 2 * (n - 1) - 1      # each pair of the call once
    # lent arrays handed back as the seed: they are copied before the call rewrites them
    lent = ctx.fill_rows_nearest("jc", 8, list(range(n)), borrow=True)
    nbr, val = ctx.fill_rows_nearest("jc", k, [], seed=lent)
    assert np.array_equal(nbr, whole.indices) and same_bits(val, whole.weights)
    # the triangular call still answers on this context
    got = ctx.fill_nearest("jc", k)
    assert np.array_equal(got[0], whole.indices) and same_bits(got[1], whole.weights)


# ---- 6: end to end ------------------------------------------------------------------------------------------------
def test_neighbors_extend_equals_de_novo(small_genomes):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    genomes, func = small_genomes, cli.METRICS["jc"]
    n = len(genomes)
    dense = golden_dense_from_file("jc", n)
    new = {11, 12}
    old = [g for k, g in enumerate(genomes) if k not in new]
    old_at = [k for k in range(n) if k not in new]
    names = [g.name for g in genomes]
    block = dense.nearest(old_at, 5)
    stored = M.NearestNeighbors([names[k] for k in old_at], block.indices, block.weights)
    want = dense.nearest(range(n), 5)
    got = M.neighbors_extend(stored, genomes, func)
    fresh = M.neighbors_de_novo(genomes, func, 5)
    for one in (got, fresh):
        assert one.nodes == names and one.is_distance and np.array_equal(one.indices, want.indices) and same_bits(one.weights, want.weights)
    assert M.LAST_FILL["metric"] == "jc" and M.LAST_FILL["n_genomes"] == n
    got = M.neighbors_extend(M.neighbors_de_novo(old, func, 5), genomes, func, k=3, verify=len(old))
    assert np.array_equal(got.indices, want.indices[:, :3]) and same_bits(got.weights, want.weights[:, :3])
    assert M.LAST_FILL["rows"] == 2
    with pytest.raises(ValueError, match="cannot decide 6"):
        M.neighbors_extend(stored, genomes, func, k=6)
    # a stored result of another metric: the guard names a pair
    other = golden_dense_from_file("gcs", n).nearest(old_at, 5)
    wrong = M.NearestNeighbors(stored.nodes, other.indices, other.weights)
    with pytest.raises(ValueError, match=r"pair \(\S+, \S+\): the nearest-neighbours list holds"):
        M.neighbors_extend(wrong, genomes, func)


def golden_dense_from_file(metric, n):
    _, values, _ = read_lower_triangle(golden_file(metric))
    return Dense(square_of(values, n, True), True)


@pytest.fixture(scope="module")
def synth200_genomes(native_built):
    from phamclust_amd.synth import synth_genomes
    return sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:200]


def test_cli_grow_nearest_reproduces_a_straight_run(synth200_genomes, tmp_path):
    from phamclust_amd.scripts import phamclust as script
    from phamclust_amd.synth import write_tsv
    genomes = synth200_genomes
    new = {3, 4, 60, 97, 131, 198, 199}
    all_tsv, old_tsv = tmp_path / "all.tsv", tmp_path / "old.tsv"
    write_tsv(genomes, all_tsv)
    write_tsv([g for k, g in enumerate(genomes) if k not in new], old_tsv)

    def run(name, tsv, *flags):
        out = tmp_path / name
        script.main([str(tsv), str(out), "-m", "jc", *flags])
        return out

    target = "nearest_jc.tsv"
    straight = run("straight", all_tsv, "--nearest", "5")
    stored = run("old", old_tsv, "--nearest", "5")
    grown = run("grown", all_tsv, "--nearest", "5", "--grow-nearest", str(stored / target))
    assert (grown / target).read_bytes() == (straight / target).read_bytes()
    assert (stored / target).read_bytes() != (straight / target).read_bytes()
    log = (grown / "phamclust.log").read_text()
    assert "grown 193 -> 200 genomes: 7 rows, " in log and "pairs filled instead of 19,900" in log
