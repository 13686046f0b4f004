"""Time the rows form of the affinity fill (pc_fill_rows_affinity) against the affinity fill from scratch: ``python tools/place_timing.py``.

One GPU, one process.  Workloads: jc on synth_real(--n, default 20000) and peq on synth_real(--n-peq, default 5000), the groups the
components at d < 0.75 cut to the --groups (default 800) largest-first labels (the smaller components share the last label), with 5 / 50
/ 500 query genomes (``--new``) spread evenly over the collection.  Every genome keeps its label, so that the rows form's result can be
held, once per workload, to the from-scratch fill's rows of the same genomes (exactly); the passes read the same elements whether a
query is labelled or not.  Per workload, call by call alternated with ``Context.fill_affinity`` from scratch on the same context -- what
a user without the rows form must run --, ``--repeats`` calls after ``--warmup``, minimum, median and every value:
  rows fill   device time of the slabs' rows fills (pc_stats.ms_total, HIP events)
  qrows       device time of k_aff_qrows over the slabs (pc_last_affinity_times' ms_rows, HIP events)
  qcols       device time of k_aff_qcols over the slabs (ms_cols; the call asks for the gain)
  finish      device time of k_aff_qfinish
  call        host clock around Context.fill_rows_affinity(want_gain=True, borrow=True), which ends synchronised
  scratch     host clock around Context.fill_affinity(borrow=True)
  ratio       scratch / call
The output is what profiles/rows_affinity_fill.txt records."""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=20000, help="genomes of the jc workload")
    ap.add_argument("--n-peq", type=int, default=5000, help="genomes of the peq workload")
    ap.add_argument("--groups", type=int, default=800, help="labels the components are cut to")
    ap.add_argument("--new", default="5,50,500", help="comma-separated counts of query genomes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_real
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    arrays = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")
    say(f"rows form of the affinity fill against the affinity fill from scratch: library version {hip.load().pc_version()}, {a.repeats} calls after "
        f"{a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    for metric, n in (("jc", a.n), ("peq", a.n_peq)):
        ctx.upload(synth_real(n), residues=metric in hip.NEEDS_RESIDUES)
        roots = ctx.fill_components(metric, 0.75)
        _, label = np.unique(roots, return_inverse=True)
        sizes = np.bincount(label)
        rank = np.empty(sizes.shape[0], dtype=np.int64)
        rank[np.argsort(-sizes, kind="stable")] = np.arange(sizes.shape[0])
        label = np.minimum(rank[label], a.groups - 1).astype(np.int32)
        g = int(label.max()) + 1
        for m in (int(x) for x in a.new.split(",")):
            rows = np.unique(np.linspace(0, n - 1, m).astype(np.int64)).astype(np.int32)
            say(f"\n{metric} synth_real({n}), {g} groups, {rows.shape[0]} query genomes: {rows.shape[0] * n:,} values filled instead of {n * (n - 1) // 2:,} "
                f"pairs; resident {16 * (rows.shape[0] * g + n) / 1e6:,.2f} MB instead of {hip.Context.affinity_bytes(n, g) / 1e6:,.2f} MB")
            got = {key: [] for key in ("fill", "rows", "cols", "finish", "call", "scratch")}
            same = None
            for step in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                found = ctx.fill_rows_affinity(metric, label, rows, g, want_gain=True, want_stats=True, borrow=True)
                call = time.perf_counter() - t0
                st = found["stats"]
                kept = [np.array(found[name]) for name in arrays]
                t0 = time.perf_counter()
                whole = ctx.fill_affinity(metric, label, g, borrow=True)
                scratch = time.perf_counter() - t0
                if same is None:
                    same = all(np.array_equal(mine, np.asarray(whole[name])[..., rows]) for mine, name in zip(kept, arrays))
                if step >= a.warmup:
                    for key, x in (("fill", st["ms_total"]), ("rows", st["ms_rows"]), ("cols", st["ms_cols"]), ("finish", st["ms_finish"]),
                                   ("call", call * 1e3), ("scratch", scratch * 1e3)):
                        got[key].append(x)
            say(f"  {st['n_slabs']} slab(s); the rows form and the from-scratch fill's rows agree: {same}")
            for key, title in (("fill", "rows fill (device)"), ("rows", "qrows (device)"), ("cols", "qcols (device)"), ("finish", "finish (device)"),
                               ("call", "call wall"), ("scratch", "from-scratch call wall")):
                say(f"    {title:<24}{spread(got[key])}")
            say(f"    ratio scratch / call    min {min(got['scratch']) / min(got['call']):.1f}x   median "
                f"{statistics.median(got['scratch']) / statistics.median(got['call']):.1f}x")
    ctx.close()
    if a.out:
        with open(a.out, "w") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
