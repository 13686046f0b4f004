"""The three bodies that run the DP cell -- pc_nw_body (tier and wide kernels) and both forms of k_nw_strip -- at the smallest shapes
at which the cell's issue-policy windows (pc_nw_systolic.h: PC_ISSUE_POLICY, PC_START_PHASE) could go wrong: the s_setprio that
bracket the cell's cheap instructions sit inside its asm blocks, next to the base step and RESET paths, the rule-3 cell has one
instruction more than the others, and a strip wave publishes its progress right behind the cells of a row step.  A priority cannot
change a value, so whichever policy the library is compiled with, every alignment's (n_ident, aln_len) equals the oracle's.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Tier kernels, in a process of its own per cell (PC_INC16 is read once).  Column genes of 60, 207, 420 and 800 residues, each
# four times over (distinct sequences) with buckets of 1, 3, 5 and 40 rows:
# * forced variants W = 4, 11, 16, 22 (one per register tier; a forced variant keeps its class's workgroup shape): one launch per
#   tier over the column genes that fit its 64 W columns.  40 rows fill every wave and put several alignments into a row stream (the
#   base step and RESET run between them); 5 rows against 420 columns at W = 11 are an 8-wave workgroup of which 3 waves have rows;
# * the automatic variant: buckets of 1 and 3 rows become one- and two-wave tasks (60 ... 420 columns), 40 rows the class's own.
# Tie rules 0 and 3 (3 is cyclic: its cell starts with one more v_add); half of the sequences over a three-letter alphabet, so that
# most pairs have co-optimal alignments for the rule to decide.
_TIER_CHECK = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import oracle as O
from phamclust_amd import hip
from phamclust_amd.genome import Genome
from phamclust_amd.pack import pack_genomes
LENS, BUCKETS = (60, 207, 420, 800), (1, 3, 5, 40)
rng = np.random.default_rng(606)
full, few = np.array(list("ACDEFGHIKLMNPQRSTVWY")), np.array(list("AGS"))
def rand(n, alpha): return "".join(alpha[rng.integers(0, alpha.size, n)])
g, h = Genome("cols"), Genome("rows")
col_len, col_bucket = [], []
for ln in LENS:
    for r in BUCKETS:
        g.add(f"c{len(col_len):02d}", rand(ln, few if len(col_len) % 2 else full))
        col_len.append(ln); col_bucket.append(r)
ncol = len(col_len)
for i in range(max(BUCKETS)):                          # rows: homologs of some column gene, cut and spliced, 1 ... ~800 residues
    base = g.phams[f"c{int(rng.integers(0, ncol)):02d}"][0]
    cut = int(rng.integers(0, len(base)))
    h.add(f"r{i:02d}", (base[:cut] + rand(int(rng.integers(0, 4)), few if i % 3 else full) + base[cut + int(rng.integers(0, 3)):]) or "M")
pk = pack_genomes([g, h])
lens = np.diff(pk.seq_off)
assert lens[:ncol].tolist() == col_len
ctx = hip.Context(0)
ctx.upload(pk)
bad = 0
for rule in (0, 3):
    ctx.set_tie_rule(rule); O.set_tie_rule(rule)
    for w in (4, 11, 16, 22, 0):
        cols = [c for c in range(ncol) if w == 0 or col_len[c] <= 64 * w]
        a = np.concatenate([ncol + (np.arange(col_bucket[c]) * 7 + c) % max(BUCKETS) for c in cols]).astype(np.int32)
        b = np.concatenate([np.full(col_bucket[c], c) for c in cols]).astype(np.int32)
        ident, diag = ctx.align_pairs(a, b, variant=w)
        _, wi, wd = O.nw_batch(pk.residues, pk.seq_off, a, b)
        alen, want_alen = lens[a] + lens[b] - diag, lens[a] + lens[b] - wd
        ok = bool(np.array_equal(ident, wi) and np.array_equal(alen, want_alen))
        bad += not ok
        print("rule", rule, "w", w, "pairs", a.size, "ok" if ok else "MISMATCH at %s" % np.flatnonzero((ident != wi) | (alen != want_alen))[:8].tolist(), flush=True)
O.set_tie_rule(0)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("inc16", ["0", "1"])
def test_tier_bodies_both_cells(native_built, inc16):
    env = dict(os.environ, PC_INC16=inc16)
    for name in ("PC_SMALL_MODES", "PC_FUSE", "PC_PIPE"):
        env.pop(name, None)
    p = subprocess.run([sys.executable, "-c", _TIER_CHECK, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.count(" ok") == 10                # 2 rules x (4 forced variants + the automatic one)


@pytest.fixture(scope="module")
def strip_case(native_built):
    """A column gene of 2,100 residues (a wide variant's ordinary class) with a bucket of ONE row and, as a second gene, of TWO: such
    tasks run strip-mined on narrow passes -- five passes of 64 x 8 columns in a one-wave workgroup, three of 64 x 12 in a two-wave
    one.  Rows are homologs of ~2,000 residues: every pass reads the boundary line the pass before wrote.  Oracle results once."""
    from oracle import oracle as O
    from phamclust_amd import hip
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    assert hip.Context.task_shape(2100, 8)["passes"] == 5 and hip.Context.task_shape(2100, 12)["passes"] == 3
    rng = np.random.default_rng(2100)
    aa = np.array(list("ACDEFGHIKLMNPQRSTVWY"))

    def rand(n): return "".join(aa[rng.integers(0, 20, n)])

    def homolog(s):
        cut = int(rng.integers(100, len(s) - 100))
        return s[:cut] + rand(int(rng.integers(1, 30))) + s[cut + int(rng.integers(20, 150)):]

    g = Genome("g")
    c1, c2 = rand(2100), rand(2100)
    for name, s in (("c1", c1), ("c2", c2), ("r1", homolog(c1)), ("r2a", homolog(c2)), ("r2b", homolog(c2)[:1500])):
        g.add(name, s)
    pk = pack_genomes([g])
    a = np.array([2, 3, 4], dtype=np.int32)            # rows
    b = np.array([0, 1, 1], dtype=np.int32)            # columns: a bucket of one row, a bucket of two
    O.set_tie_rule(0)
    _, wi, wd = O.nw_batch(pk.residues, pk.seq_off, a, b)
    return pk, a, b, wi, wd


@pytest.mark.parametrize("pipe", ["0", "4"])
def test_strip_bodies(gpu_ctx, strip_case, pipe):
    """PC_PIPE=0: one row per wave.  PC_PIPE=4: the passes of each alignment over four waves, every wave reading the line of the wave
    before it while that wave writes it -- the progress word must still follow the boundary stores it announces."""
    pk, a, b, wi, wd = strip_case
    lens = np.diff(pk.seq_off)
    try:
        os.environ["PC_PIPE"] = pipe
        gpu_ctx.set_tie_rule(0)
        gpu_ctx.upload(pk)
        ident, diag = gpu_ctx.align_pairs(a, b)
    finally:
        os.environ.pop("PC_PIPE", None)
    assert np.array_equal(ident, wi), f"PC_PIPE {pipe}"
    assert np.array_equal(lens[a] + lens[b] - diag, lens[a] + lens[b] - wd), f"PC_PIPE {pipe}"

