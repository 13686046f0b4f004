"""The aligner at the limits it documents (run with ``-m gpu`` on the MI355X box).

* genes of 65,535 residues (pc_upload's limit): the compare cell keeps (n_ident | n_diag << 16) in one 32-bit word, which
  identical 65,535-residue genes fill to exactly 0xFFFFFFFF; the score headroom (PC_BASE_STEP) and the "-inf" bound (PC_NEG4)
  are argued for la <= 65,535 only; the refusal at 65,536;
* percent-positives across the profile cell's 13-bit fields (n_ident | n_diag << 13: strip-mined up to 8,191 columns, the
  general kernel beyond);
* a row stream that carries a full task's share of alignments (PC_TASK_ROWS / PC_MIN_WAVES = 52), never cleared in between;
* strip-pass edges (passes of 64 W columns) and the row-staging windows (PC_STRIP_WIN = 32, PC_STRIP_BND = 64).

Every expected value is the CPU oracle's (oracle.nw_batch / oracle.fill) or a closed form argued where it is used.  In
``align_pairs(a, b)`` gene a is the row (query) and gene b the column: the column gene is what the kernel spreads over its
lanes and cuts into passes.
"""

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 65535                                                      # pc_upload's gene-length limit (pc_upload.hip, upload_sets)
AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def _oracle():
    from oracle import oracle
    return oracle


def _workers():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _rand(rng, n):
    return AA[rng.integers(0, AA.size, n)].tobytes().decode()


def _mutated(rng, seq, sub=0.1, indel=0.01):
    """Substitutions at rate ``sub``, deletions and insertions at rate ``indel`` each."""
    a = np.frombuffer(seq.encode(), dtype=np.uint8).copy()
    hit = rng.random(a.size) < sub
    a[hit] = AA[rng.integers(0, AA.size, int(hit.sum()))]
    a = a[rng.random(a.size) >= indel]
    n_ins = int((rng.random(a.size) < indel).sum())
    a = np.insert(a, np.sort(rng.integers(0, a.size + 1, n_ins)), AA[rng.integers(0, AA.size, n_ins)])
    return a.tobytes().decode()


def _substituted(rng, seq, sub=0.15):
    """Substitutions only: the length stays."""
    return _mutated(rng, seq, sub=sub, indel=0.0)


def _pack_one_genome(seqs):
    """One genome, gene i = seqs[i] (pham names sort in list order)."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    g = Genome("g")
    for i, s in enumerate(seqs):
        g.add(f"p{i:04d}", s)
    pk = pack_genomes([g])
    assert np.array_equal(np.diff(pk.seq_off), [len(s) for s in seqs])
    return pk


def _nw(pk, a, b, workers=None):
    """oracle.nw_batch, the pairs dealt over threads one by one (its own OpenMP loop deals them in chunks of 16, which
    leaves a few long pairs on one thread).  Returns (n_ident, n_diag)."""
    O = _oracle()
    a = np.asarray(a, dtype=np.int32)
    b = np.asarray(b, dtype=np.int32)
    lens = np.diff(pk.seq_off)
    order = np.argsort(-(lens[a] * lens[b]), kind="stable")
    workers = workers or _workers()
    groups = [order[k::4 * workers] for k in range(min(order.size, 4 * workers))]
    ident, diag = np.zeros(a.size, np.int32), np.zeros(a.size, np.int32)

    def run(idx):
        _, wi, wd = O.nw_batch(pk.residues, pk.seq_off, a[idx], b[idx], nthreads=1)
        return idx, wi, wd

    with ThreadPoolExecutor(workers) as pool:
        for idx, wi, wd in pool.map(run, groups):
            ident[idx], diag[idx] = wi, wd
    return ident, diag


def _set_pipe(pipe):
    if pipe is None:
        os.environ.pop("PC_PIPE", None)
    else:
        os.environ["PC_PIPE"] = pipe


# ---------------------------------------------------------------------------------------------------------------------
# 65,535-residue genes
# ---------------------------------------------------------------------------------------------------------------------
SHORT_COLUMNS = (1, 2, 63, 64, 65, 1536, 4096)                 # in-register tiers: 1 lane ... 64 lanes of W = 64
PREFIX_CUTS = (1, 7, 64)
W_SHORT = 50000


class LongGenes:
    def __init__(self):
        rng = np.random.default_rng(65535)
        x = _rand(rng, L)
        h = _mutated(rng, x)[:L]                               # a random homolog, at most L residues
        seqs = {"X": x, "H": h, "W": "W" * L, "S": "*" * L, "Wshort": "W" * W_SHORT}
        for k in PREFIX_CUTS:
            seqs[f"X-{k}"] = x[:L - k]
        for m in SHORT_COLUMNS:                                # short columns: a homologous window of X, poly-W, poly-*
            at = int(rng.integers(0, L - m))
            seqs[f"frag{m}"] = _mutated(rng, x[at:at + m]) or x[at]
            seqs[f"W{m}"] = "W" * m
            seqs[f"S{m}"] = "*" * m
        self.names = list(seqs)
        self.gene = {name: i for i, name in enumerate(self.names)}
        self.pk = _pack_one_genome([seqs[n] for n in self.names])
        # the two random-homolog 65,535 x 65,535 pairs are the only such pairs the oracle aligns (~30 s each on one core):
        # started here, in the background, so that they run while the other tests use the GPU
        self._pool = ThreadPoolExecutor(1)
        self.homolog_pairs = [("H", "X"), ("X", "H")]
        a, b = self.idx(self.homolog_pairs)
        self.homolog_want = self._pool.submit(_nw, self.pk, a, b, 2)

    def idx(self, pairs):
        return (np.array([self.gene[r] for r, _ in pairs], dtype=np.int32), np.array([self.gene[c] for _, c in pairs], dtype=np.int32))

    def close(self):
        self._pool.shutdown(wait=True)


@pytest.fixture(scope="module")
def long_genes(native_built):
    lg = LongGenes()
    yield lg
    lg.close()


def test_65535_residue_rows_on_the_in_register_tiers(gpu_ctx, long_genes):
    """Rows of 65,535 residues (random, its homolog, poly-W, poly-*) against column genes of 1, 2, 63, 64, 65, 1,536 and
    4,096 residues (one lane of W = 2 ... 64 lanes of W = 64): stream entries of the longest row the upload admits, the
    score bias (+1 per anti-diagonal) at its largest, and the "virtual row -1" reset after such a row.  Oracle-checked."""
    lg = long_genes
    rows = ("X", "H", "W", "S")
    cols = [f"{kind}{m}" for m in SHORT_COLUMNS for kind in ("frag", "W", "S")]
    pairs = [(r, c) for r in rows for c in cols]
    a, b = lg.idx(pairs)
    want_i, want_d = _nw(lg.pk, a, b)
    gpu_ctx.upload(lg.pk)
    try:
        for pipe in ("0", None):
            _set_pipe(pipe)
            ident, diag = gpu_ctx.align_pairs(a, b)
            assert np.array_equal(ident, want_i) and np.array_equal(diag, want_d), f"PC_PIPE {pipe}"
    finally:
        os.environ.pop("PC_PIPE", None)
    # poly-W rows against poly-W columns: every column residue on the diagonal, one gap run (the closed form of the
    # column tests below, with the roles swapped)
    for k, (r, c) in enumerate(pairs):
        if r == "W" and c.startswith("W"):
            m = int(c[1:])
            assert (ident[k], diag[k]) == (m, m), (r, c)


def test_fills_of_a_collection_with_65535_residue_genes(gpu_ctx, native_built):
    """aai and peq fills of three genomes holding 65,535-residue genes, as rows (the source genome's gene of a shared pham
    is the row: anchor rule, tie -> source) and as columns, against shorter genes of the other genomes; equal to the
    oracle.  (No 65,535 x 65,535 pair: the oracle aligns those at ~30 s each.)"""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    O = _oracle()
    rng = np.random.default_rng(3)
    x = _rand(rng, L)
    g0, g1, g2 = Genome("g0"), Genome("g1"), Genome("g2")
    g0.add("pA", x)
    g0.add("pB", "W" * 100)
    g1.add("pA", _mutated(rng, x[20000:24500]))
    g1.add("pC", "*" * 1200)
    g1.add("pD", _rand(rng, 300))
    g2.add("pA", _mutated(rng, x[:1536]))
    g2.add("pB", "W" * L)
    g2.add("pC", "W" * L)
    g2.add("pD", _rand(rng, 280))
    pk = pack_genomes([g0, g1, g2])
    assert np.diff(pk.seq_off).max() == L
    with ThreadPoolExecutor(2) as pool:                                                # two single-threaded oracle fills side by side
        want = {m: pool.submit(O.fill, pk, m, True, 1) for m in ("aai", "peq")}
        gpu_ctx.upload(pk)
        got = {m: gpu_ctx.fill(m) for m in ("aai", "peq")}
        for m in ("aai", "peq"):
            assert np.array_equal(got[m], want[m].result()), m


def test_gene_length_refused_at_65536(gpu_ctx, native_built):
    """pc_upload admits genes of up to 65,535 residues.  One of 65,536 is refused -- with and without the residues -- by
    an error that names the gene and the limit, and leaves no collection behind (a fill then fails rather than serve
    the previous upload); the same context then takes a valid upload, 65,535 residues included (also without the
    residues, which then follow on the first aai fill), and fills what the oracle fills."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.hip import HipLibraryError
    from phamclust_amd.pack import pack_genomes
    O = _oracle()
    rng = np.random.default_rng(65536)
    long_seq = _rand(rng, L + 1)

    def collection(long_len):
        g0, g1 = Genome("g0"), Genome("g1")
        g0.add("pA", long_seq[:50])
        g0.add("pB", _rand(np.random.default_rng(1), 200))
        g1.add("pB", _rand(np.random.default_rng(2), 190))
        g1.add("pA", long_seq[:long_len])
        g1.add("pC", "MKV")
        return pack_genomes([g0, g1])

    bad, ok = collection(L + 1), collection(L)
    k_bad = int(np.flatnonzero(np.diff(bad.seq_off) > L)[0])
    want = {m: O.fill(ok, m) for m in ("aai", "jc")}
    for residues in (True, False):
        with pytest.raises(HipLibraryError) as err:
            gpu_ctx.upload(bad, residues=residues)
        msg = str(err.value)
        assert f"gene {k_bad} has length {L + 1}" in msg and f"limit {L}" in msg, msg
        with pytest.raises(HipLibraryError):
            gpu_ctx.fill("jc")
        gpu_ctx.upload(ok, residues=residues)
        assert np.array_equal(gpu_ctx.fill("jc"), want["jc"]), residues
        assert np.array_equal(gpu_ctx.fill("aai"), want["aai"]), residues


# ---------------------------------------------------------------------------------------------------------------------
# percent-positives across the 13-bit edge
# ---------------------------------------------------------------------------------------------------------------------
PPOS_STRIP = (1536, 1537, 3072, 3073, 6144, 7680, 7681, 8191)          # 64 x 24 = 1,536-column passes; 8,191 = 0x1FFF
PPOS_GENERAL = (8192, 9000)


def _ppos_collection(rng, lengths, row_len):
    """Genome "a" holds one row gene per length, genome "b<L>" the column gene of L residues in the same pham: every pair
    (a, b<L>) is ONE alignment, and its column is b<L>'s gene -- each genome holds one gene of the pham, so the anchor (the
    genome with fewer genes, tie -> the source, metrics.py:208-209; pc_walk.hip pc_visit) is the source "a", whose gene is
    the row (pc_plan.hip: the column sequence is the other side of the key).  The b genomes share no pham with each other,
    except the identical / mutated 8,191-residue pair (both columns at most 8,191)."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    a = Genome("a")
    bs = []
    for k, n in enumerate(lengths):
        col = _rand(rng, n)
        b = Genome(f"b{k:02d}_{n}")
        b.add(f"p{k:02d}", col)
        bs.append(b)
        a.add(f"p{k:02d}", row_len(n, col))
        if n == 8191:                                          # the same row against its identical column (n_ident = 8,191:
            b2 = Genome(f"b{k:02d}_{n}m")                      # the 13-bit field full) and against a mutated copy
            b2.add(f"p{k:02d}", _substituted(rng, col))
            bs.append(b2)
    return pack_genomes(sorted([a] + bs, key=lambda g: g.name))


def test_percent_positives_across_the_13_bit_edge(gpu_ctx, native_built):
    """fill("aai_ppos"): column genes of 1,536 ... 8,191 residues run strip-mined on the profile cell (W = 24, whose
    statistics are 13-bit fields: pc_nw_ppos_systolic, PC_STRIP_PPOS_MAX_LB), 8,192 and 9,000 on the general kernel (short
    rows there: one lane per alignment).  Each collection keeps its column genes on one side of the edge -- the route is
    taken per launch class from the class's LONGEST column gene, so an 8,192 would drag a class-mate of 8,191 along."""
    from phamclust_amd.hip import Context
    O = _oracle()
    rng = np.random.default_rng(8191)
    route = {n: Context.ppos_width(n) for n in PPOS_STRIP + PPOS_GENERAL}
    assert all(route[n] == 24 for n in PPOS_STRIP) and all(route[n] == 0 for n in PPOS_GENERAL), route
    print("\npercent-positives: " + ", ".join(f"{n} -> " + ("strip W = 24" if route[n] else "general kernel") for n in route))
    strip = _ppos_collection(rng, PPOS_STRIP, lambda n, col: col if n == 8191 else _mutated(rng, col, sub=0.2, indel=0.005))
    general = _ppos_collection(rng, PPOS_GENERAL, lambda n, col: _mutated(rng, col[n // 3:n // 3 + 240]))
    got = {}
    for name, pk in (("strip", strip), ("general", general)):
        gpu_ctx.upload(pk)
        got[name] = gpu_ctx.fill("aai_ppos", as_distance=False)
        assert np.array_equal(got[name], O.fill(pk, "aai_ppos", as_distance=False)), name
    names = strip.names
    i_a, i_b = names.index("a"), next(i for i, n in enumerate(names) if n.endswith("_8191"))
    assert got["strip"][i_a * len(names) - i_a * (i_a + 1) // 2 + (i_b - i_a - 1)] == 1.0   # the identical 8,191 pair: 8191 / 8191


# ---------------------------------------------------------------------------------------------------------------------
# a full row stream
# ---------------------------------------------------------------------------------------------------------------------
def test_full_row_stream_of_long_rows(gpu_ctx, native_built):
    """52 alignments back to back in every row stream, never cleared in between (each starts PC_BASE_STEP above the one
    before): a 100-residue column gene on a forced narrow variant (W = 2 and 3: 50 and 34 lanes, so one segment per wave),
    208 rows in one task of 4 waves.  The rows, of up to 65,535 residues, alternate high-scoring (the column embedded in
    a long row, poly-W against a poly-W column) and low-scoring (unrelated, poly-*).  Oracle-checked."""
    from phamclust_amd.hip import Context
    rng = np.random.default_rng(52)
    n_rows = 208
    for w in (2, 3):
        shape = Context.task_shape(100, w)
        assert shape["streams"] == 1 and shape["rows"] == n_rows and shape["passes"] == 0, shape
        per_stream = shape["rows"] // (shape["waves"] * shape["streams"])
        assert per_stream == 52 and per_stream * shape["waves"] == n_rows, shape
    print(f"\nrow stream: {per_stream} alignments per stream ({n_rows} rows, {shape['waves']} waves, 1 stream per wave)")
    col = _rand(rng, 100)
    lens = [L, 1, 40000, 100, L, 7, 30000, 2000, L - 1, 150, 12000, 64]
    rows = []
    for i in range(n_rows):
        n = lens[i % len(lens)] if i % 5 else int(rng.integers(1, L + 1))
        if i % 2 == 0:                                          # high: the column (mutated) inside a long row, or poly-W
            if i % 4 == 0:
                core = _mutated(rng, col, sub=0.05, indel=0.0)
                at = int(rng.integers(0, max(1, n - 100)))
                rows.append((_rand(rng, at) + core + _rand(rng, max(0, n - at - 100)))[:max(n, 1)] or "W")
            else:
                rows.append("W" * n)
        else:                                                   # low: unrelated or poly-*
            rows.append(_rand(rng, n) if i % 4 == 1 else "*" * n)
    seqs = [col, "W" * 100] + rows
    pk = _pack_one_genome(seqs)
    assert max(len(r) for r in rows) == L
    a = np.tile(np.arange(2, 2 + n_rows, dtype=np.int32), 2)
    b = np.repeat(np.array([0, 1], dtype=np.int32), n_rows)   # each column gene: one bucket of 208 rows = one full task
    want_i, want_d = _nw(pk, a, b)
    gpu_ctx.upload(pk)
    for w in (2, 3):
        ident, diag = gpu_ctx.align_pairs(a, b, variant=w)
        assert np.array_equal(ident, want_i) and np.array_equal(diag, want_d), w


# ---------------------------------------------------------------------------------------------------------------------
# strip-pass and staging edges
# ---------------------------------------------------------------------------------------------------------------------
EDGE_ROWS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97)            # around PC_STRIP_WIN = 32 and PC_STRIP_BND = 64


def _edge_rows(rng, col):
    """Rows of EDGE_ROWS residues cut from the column (with substitutions) and one row longer than the column."""
    out = []
    for m in EDGE_ROWS:
        at = int(rng.integers(0, len(col) - m + 1))
        out.append(_substituted(rng, col[at:at + m], sub=0.2))
    longer = _mutated(rng, col, sub=0.1, indel=0.004)
    out.append((longer + _rand(rng, len(col) + 37))[:len(col) + 37])
    return out


def test_strip_pass_and_staging_edges(gpu_ctx, native_built):
    """Column genes of k x 64 W and k x 64 W + 1 residues (k = 2, 3) on the wide variants forced (W = 32, 48, 64), and of
    4,608 / 4,609 / 6,144 / 6,145 residues in tasks of one and of two rows (the automatic choice: passes of 512 resp. 768
    columns, W = 8 / 12; 4,608 = 9 x 512 = 6 x 768, 6,144 = 12 x 512 = 8 x 768), each against rows around the staging
    windows and one row longer than the column; under PC_PIPE=0 (one row per wave) and unset (pipelined).  Oracle-checked."""
    from phamclust_amd.hip import Context
    rng = np.random.default_rng(64)
    seqs, forced, narrow, oracle_col = [], {}, [], []

    def add(s):
        seqs.append(s)
        return len(seqs) - 1

    for w in (32, 48, 64):
        pairs = []
        for k in (2, 3):
            for n in (k * 64 * w, k * 64 * w + 1):
                assert Context.task_shape(n, w)["passes"] == (k if n == k * 64 * w else k + 1)
                col = _rand(rng, n)
                c = add(col)
                pairs += [(add(r), c) for r in _edge_rows(rng, col)]
        forced[w] = pairs
    for n in (4608, 4609, 6144, 6145):
        assert Context.task_shape(n, 0)["passes"] > 0                                  # strip-mined under the chooser
        col = _rand(rng, n)
        c = add(col)
        rows = [add(r) for r in _edge_rows(rng, col)]
        for per_task in (1, 2):                                  # a copy of the column per task: buckets of one / two rows
            for t in range(0, len(rows), per_task):
                cc = add(col)
                for r in rows[t:t + per_task]:
                    narrow.append((r, cc))
                    oracle_col.append(c)
    pk = _pack_one_genome(seqs)
    all_pairs = [p for w in (32, 48, 64) for p in forced[w]]
    a_all = np.array([r for r, _ in all_pairs] + [r for r, _ in narrow], dtype=np.int32)
    b_all = np.array([c for _, c in all_pairs] + oracle_col, dtype=np.int32)          # (the narrow copies are the same sequence)
    want_i, want_d = _nw(pk, a_all, b_all)
    gpu_ctx.upload(pk)
    try:
        for pipe in ("0", None):
            _set_pipe(pipe)
            at = 0
            for w in (32, 48, 64):
                a = np.array([r for r, _ in forced[w]], dtype=np.int32)
                b = np.array([c for _, c in forced[w]], dtype=np.int32)
                ident, diag = gpu_ctx.align_pairs(a, b, variant=w)
                sel = slice(at, at + a.size)
                assert np.array_equal(ident, want_i[sel]) and np.array_equal(diag, want_d[sel]), (w, pipe)
                at += a.size
            a = np.array([r for r, _ in narrow], dtype=np.int32)
            b = np.array([c for _, c in narrow], dtype=np.int32)
            ident, diag = gpu_ctx.align_pairs(a, b)
            assert np.array_equal(ident, want_i[at:]) and np.array_equal(diag, want_d[at:]), ("one / two rows", pipe)
    finally:
        os.environ.pop("PC_PIPE", None)


# ---------------------------------------------------------------------------------------------------------------------
# 65,535-residue column genes (last: the oracle's two long pairs have been running in the background since the first test)
# ---------------------------------------------------------------------------------------------------------------------
def _closed_form_column_pairs():
    """(row, column, n_ident, n_diag) with a 65,535-residue (or 50,000+) column gene, whose statistics are the same for every
    co-optimal alignment -- so for every tie rule:
    * X against itself and X against its prefixes X[:L-k] (either role): BLOSUM62's diagonal beats every other entry of its
      row (S(a, a) >= 4 > 3 >= S(a, b)), so a path scores at most sum S(x_j, x_j) over the shorter sequence minus one gap run
      of the length difference; reaching it needs n_diag = the shorter length, every diagonal pair identical and one gap
      run, hence (L-k, L-k); k = 0: no gap, (L, L) -- which fills the compare cell's 16-bit fields to 0xFFFF each;
    * poly-W against poly-W of the same or a shorter length (either role): the same argument with S(W, W) = 11 (the highest
      score the kernel can meet, 11 x 65,535), (L_short, L_short);
    * poly-W against poly-* (either role): S(W, *) = -4.  With d diagonal steps both sequences carry L - d gap residues,
      i.e. at least two gap runs: score <= -4 d - 2 (11 + L - d - 1) = -2 (L + 10) - 2 d, so every optimum has d = 0: (0, 0),
      two gap runs of 65,535 residues, the E / F states extended 65,535 times."""
    out = [("X", "X", L, L), ("W", "W", L, L), ("Wshort", "W", W_SHORT, W_SHORT), ("W", "Wshort", W_SHORT, W_SHORT),
           ("W", "S", 0, 0), ("S", "W", 0, 0)]
    for k in PREFIX_CUTS:
        out += [(f"X-{k}", "X", L - k, L - k), ("X", f"X-{k}", L - k, L - k)]
    return out


def test_65535_residue_columns_on_the_strip_kernel(gpu_ctx, long_genes):
    """Column genes of 65,535 residues, strip-mined: the wide variants forced under PC_PIPE=0 (one row per wave; 32 / 22 / 16
    passes of 2,048 / 3,072 / 4,096 columns) and the automatic choice pipelined (PC_PIPE unset: 8 waves; 4; 3, which does
    not divide the 128 passes of 512 columns), tie rule 0; the automatic choice again under tie rule 3 (two "open" tags).
    Closed forms (_closed_form_column_pairs) and two random-homolog pairs against the oracle."""
    from phamclust_amd.hip import Context
    lg = long_genes
    closed = _closed_form_column_pairs()
    pairs = [(r, c) for r, c, _, _ in closed] + lg.homolog_pairs
    a, b = lg.idx(pairs)
    n_closed = len(closed)
    want_i = np.array([i for _, _, i, _ in closed] + [0] * len(lg.homolog_pairs), dtype=np.int32)
    want_d = np.array([d for _, _, _, d in closed] + [0] * len(lg.homolog_pairs), dtype=np.int32)
    passes = {w: Context.task_shape(L, w)["passes"] for w in (32, 48, 64)}
    assert passes == {32: 32, 48: 22, 64: 16}
    assert Context.task_shape(L, 0)["passes"] > 0                                      # the chooser strip-mines it too
    print(f"\n65,535 columns: strip passes per forced width {passes}; pipelined: {-(-L // 512)} passes of 512 columns")
    runs = [(0, "0", w) for w in (32, 48, 64)] + [(0, pipe, 0) for pipe in (None, "4", "3")] + [(3, None, 0)]
    got = {}
    gpu_ctx.upload(lg.pk)
    try:
        for rule, pipe, variant in runs:
            gpu_ctx.set_tie_rule(rule)
            _set_pipe(pipe)
            sel = slice(None) if rule == 0 else slice(0, n_closed)                     # the homologs' optimum depends on the rule
            ident, diag = gpu_ctx.align_pairs(a[sel], b[sel], variant=variant)
            tag = f"rule {rule} PC_PIPE {pipe} variant {variant}"
            for k in range(n_closed):
                assert (ident[k], diag[k]) == (want_i[k], want_d[k]), (tag, pairs[k], ident[k], diag[k])
            got[(rule, pipe, variant)] = (ident[n_closed:], diag[n_closed:])
    finally:
        os.environ.pop("PC_PIPE", None)
        gpu_ctx.set_tie_rule(0)
    hom_i, hom_d = lg.homolog_want.result()
    assert (hom_d > 50000).all() and (hom_i < hom_d).all()                             # really homologs, really not identical
    for key, (ident, diag) in got.items():
        if key[0] == 0:
            assert np.array_equal(ident, hom_i) and np.array_equal(diag, hom_d), key
