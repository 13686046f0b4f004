"""pc_nw_body's row-stream upkeep -- the staging of a stream window and the schedule of flag events it builds (pc_nw_events.h) --
at the smallest shapes at which it can go wrong.  The step loop no longer looks at an entry's flags unless the schedule says that
this step has an event, so a bit placed one step or one window off loses a RESET (the alignment then starts on the scores of the
one before) or an output (the result slot keeps what it held): every (n_ident, aln_len) is compared bit for bit with the oracle's.

* Column lengths W, 32 W, 32 W + 1 and 64 W put the output lane at k_out = 0 (the head lane itself), 31, 32 and 63, and make 16, 2, 1
  and 1 row streams per wave; W = 2 and 8, 12, 13 and 19, 24 are the narrowest and widest body of each register tier (forced; a
  forced variant keeps its class's workgroup shape: with the profile cell 8 waves for 416 columns at W = 13 and 608 at W = 19, 4 elsewhere).
* Rows of 1, 2, 31, 32, 33, 63, 64 and 65 residues, mixed within a stream: RESET and LAST sit on the first and the last entry of a
  32-entry window, and a LAST placed k_out steps later crosses one and two window boundaries.
* Per column length one bucket of the class's full task (up to 13 alignments per stream where the class holds that many rows; odd and
  even step counts as the mixes fall) and one of 5 rows (fewer rows than segments, waves without rows).
* Buckets of 1 and 3 rows under the automatic variant: the one- and two-wave task modes.
* Both cells (PC_INC16 is read once: a process each), tie rules 0 and 3, and one tiny fill per process through the planner and
  the fused tier launches: peq, and percent-positives (aai_ppos).
"""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHECK = r"""
import os, sys, numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import oracle as O
from phamclust_amd import hip
from phamclust_amd.genome import Genome
from phamclust_amd.pack import pack_genomes
WIDTHS, EDGE, NROWS = (2, 8, 12, 13, 19, 24), (1, 2, 31, 32, 33, 63, 64, 65), 208
rng = np.random.default_rng(909)
full, few = np.array(list("ACDEFGHIKLMNPQRSTVWY")), np.array(list("AGS"))
def rand(n, alpha): return "".join(alpha[rng.integers(0, alpha.size, n)])
g, h = Genome("cols"), Genome("rows")
cols = []                                              # (forced width, bucket rows)
for w in WIDTHS:
    for lb in (w, 32 * w, 32 * w + 1, 64 * w):
        shape = hip.Context.task_shape(lb, w)
        assert shape["passes"] == 0 and shape["streams"] == (16 if lb == w else 2 if lb == 32 * w else 1), (w, lb, shape)
        for bucket in (shape["rows"], 5):
            g.add(f"c{len(cols):03d}", rand(lb, few if len(cols) % 3 == 0 else full))
            cols.append((w, bucket))
assert {hip.Context.task_shape(32 * w, w)["waves"] for w in WIDTHS} == ({4, 8} if os.environ["PC_INC16"] == "1" else {4})   # (the compare cell's small profile never needs 8)
for lb in (60, 207, 420):                              # the automatic variant: one- and two-wave tasks
    for bucket in (1, 3):
        g.add(f"c{len(cols):03d}", rand(lb, few if bucket == 1 else full))
        cols.append((0, bucket))
ncol = len(cols)
assert max(b for _, b in cols) <= NROWS
row_len = [EDGE[int(rng.integers(0, 8))] for _ in range(NROWS)]   # the rows of a stream (every 4th ... 64th of a bucket) come out mixed
for i in range(NROWS):
    h.add(f"r{i:03d}", rand(row_len[i], few if i % 2 else full))
pk = pack_genomes([g, h])
lens = np.diff(pk.seq_off)
assert lens[ncol:].tolist() == row_len
ctx = hip.Context(0)
ctx.upload(pk)
bad = 0
for rule in (0, 3):
    ctx.set_tie_rule(rule); O.set_tie_rule(rule)
    for w in WIDTHS + (0,):
        mine = [c for c in range(ncol) if cols[c][0] == w]
        a = np.concatenate([ncol + (np.arange(cols[c][1]) + 11 * c) % NROWS for c in mine]).astype(np.int32)
        b = np.concatenate([np.full(cols[c][1], c) for c in mine]).astype(np.int32)
        ident, diag = ctx.align_pairs(a, b, variant=w)
        _, wi, wd = O.nw_batch(pk.residues, pk.seq_off, a, b)
        alen, want_alen = lens[a] + lens[b] - diag, lens[a] + lens[b] - wd
        ok = bool(np.array_equal(ident, wi) and np.array_equal(alen, want_alen))
        bad += not ok
        print("rule", rule, "w", w, "pairs", a.size, "ok" if ok else "MISMATCH at %s" % np.flatnonzero((ident != wi) | (alen != want_alen))[:8].tolist(), flush=True)
O.set_tie_rule(0); ctx.set_tie_rule(0)
# a tiny fill: three genomes sharing eight phams whose genes run from 2 to 300 residues (rows of a bucket: the other genomes' copies)
gs = [Genome(f"g{i}") for i in range(3)]
for p, ln in enumerate((2, 31, 33, 64, 65, 130, 207, 300)):
    base = rand(ln, full)
    for i, gg in enumerate(gs):
        cut = int(rng.integers(0, ln))
        gg.add(f"p{p}", base if i == 0 else (base[:cut] + rand(int(rng.integers(0, 3)), full) + base[cut + int(rng.integers(0, 2)):]) or "M")
pf = pack_genomes(gs)
ctx.upload(pf)
for metric in ("peq", "aai_ppos"):
    ok = bool(np.array_equal(ctx.fill(metric), O.fill(pf, metric)))
    bad += not ok
    print("fill", metric, "ok" if ok else "MISMATCH", flush=True)
sys.exit(1 if bad else 0)
"""


@pytest.mark.parametrize("inc16", ["0", "1"])
def test_stream_upkeep_both_cells(native_built, inc16):
    env = dict(os.environ, PC_INC16=inc16)
    for name in ("PC_SMALL_MODES", "PC_FUSE", "PC_PIPE"):
        env.pop(name, None)
    p = subprocess.run([sys.executable, "-c", _CHECK, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.count(" ok") == 2 * 7 + 2             # 2 rules x (6 forced widths + the automatic variant), 2 fills
