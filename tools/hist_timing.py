"""Time the distribution fill (pc_fill_hist) against the only route the commit before it offers: ``python tools/hist_timing.py``.

One GPU, one process.  Workloads: jc on synth_real(--n, default 20000) and peq on synth_real(--n-peq, default 5000), each without a
partition and with the components at d < 0.75 as the groups (the 800- / 233-group partitions of profiles/between_fill.txt).  Per
workload, ``--repeats`` calls after ``--warmup``, minimum, median and every value (ms):
  fill       device time of the slabs' fills (pc_stats.ms_total, HIP events)
  pass       device time of k_hist_pass summed over the slabs (pc_last_hist_times, HIP events), the bytes of slab per second it amounts
             to (8 bytes per pair), and its ratio to the union pass of the components fill over the same slab, measured call by call on
             the same build (pc_last_component_times) -- profiles/components_fill.txt records 0.53 ms for it under jc at N = 20,000
  finish     device time of k_hist_finish (HIP events)
  d2h        call - (fill + pass + finish): the copy of the bins, the host's sum over them and the launches' own cost
  call       host clock around Context.fill_hist(borrow=True), which ends synchronised
and, alternated with it call by call on the same context:
  dense      host clock around Context.fill(borrow=True) -- the whole fill and its D2H copy -- then np.rint and np.bincount on the host
  ratio      dense / call
The two histograms are compared once per workload, exactly.  The output is what profiles/hist_fill.txt records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


RECORDED_UNION_MS = 0.53           # profiles/components_fill.txt: the union pass over 1.6 GB of slab, jc at N = 20,000, d < 0.75


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  spread {max(xs) - min(xs):8.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=20000, help="genomes of the jc workloads")
    ap.add_argument("--n-peq", type=int, default=5000, help="genomes of the peq workloads")
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

    say(f"distribution fill against dense fill + D2H + host rint + bincount: library version {hip.load().pc_version()}, table "
        f"{hip.Context.hist_table_slots()} slots, {hip.Context.hist_probes()} probes, {a.repeats} calls after {a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    for metric, n in (("jc", a.n), ("peq", a.n_peq)):
        pairs = n * (n - 1) // 2
        ctx.upload(synth_real(n), residues=metric in hip.NEEDS_RESIDUES)
        roots = ctx.fill_components(metric, 0.75)
        _, label = np.unique(roots, return_inverse=True)
        label = label.astype(np.int32)
        for group in (None, label):
            g = 0 if group is None else int(group.max()) + 1
            say(f"\n{metric} {'no partition' if group is None else f'{g} groups (components at d < 0.75)'}: synth_real({n}), {pairs:,} pairs, "
                f"dense vector {pairs * 8 / 1e6:,.1f} MB, histogram {(1 if group is None else 2) * hip.HIST_BINS * 8 / 1e6:.1f} MB")
            got = {key: [] for key in ("fill", "pass", "finish", "d2h", "call", "dense", "union")}
            same = None
            for step in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                hist, st = ctx.fill_hist(metric, group, g or None, want_stats=True, borrow=True)
                call = (time.perf_counter() - t0) * 1e3
                kept = np.array(hist)
                t0 = time.perf_counter()
                condensed = np.asarray(ctx.fill(metric, borrow=True))
                dense = np.bincount(np.rint(condensed * 1.0e6).astype(np.int64), minlength=hip.HIST_BINS)
                dense_ms = (time.perf_counter() - t0) * 1e3
                if same is None:
                    same = bool(np.array_equal(kept.sum(axis=0), dense))
                _, cst = ctx.fill_components(metric, 0.75, want_stats=True)
                if step >= a.warmup:
                    for key, x in (("fill", st["ms_total"]), ("pass", st["ms_pass"]), ("finish", st["ms_finish"]), ("call", call), ("dense", dense_ms),
                                   ("d2h", call - st["ms_total"] - st["ms_pass"] - st["ms_finish"]), ("union", cst["ms_union"])):
                        got[key].append(x)
            rate = pairs * 8 / (min(got["pass"]) * 1e-3) / 1e12 if min(got["pass"]) > 0 else 0.0
            say(f"  {st['n_slabs']} slab(s), {int((kept.sum(axis=0) > 0).sum()):,} occupied bins, the largest {int(kept.sum(axis=0).max()) / pairs:.1%} of the "
                f"pairs; the two routes agree on the histogram: {same}")
            say(f"    fill (device)         {spread(got['fill'])}")
            say(f"    hist: pass            {spread(got['pass'])}   = {rate:.2f} TB/s of slab")
            say(f"    union pass, same slab {spread(got['union'])}   pass / union = {min(got['pass']) / min(got['union']):.2f}")
            if metric == "jc" and n == 20000:
                say(f"    pass / the union pass profiles/components_fill.txt records for jc at N = 20,000 ({RECORDED_UNION_MS} ms) = "
                    f"{min(got['pass']) / RECORDED_UNION_MS:.2f}")
            say(f"    hist: finish          {spread(got['finish'])}")
            say(f"    hist: D2H and host    {spread(got['d2h'])}")
            say(f"    hist: call            {spread(got['call'])}")
            say(f"    dense route: fill+D2H+rint+bincount {spread(got['dense'])}")
            say(f"    ratio dense / call    min {min(got['dense']) / min(got['call']):.1f}x   median "
                f"{statistics.median(got['dense']) / statistics.median(got['call']):.1f}x;   pass / fill = {min(got['pass']) / min(got['fill']):.2f}")
    ctx.close()
    if a.out:
        with open(a.out, "w") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
