"""Time the pair-list fill (pc_fill_pairs) and the af bound of peq edge lists: ``python tools/pairs_timing.py`` writes
``profiles/pairs_fill.txt``.

One process, one GPU.  Per workload -- ``synth_real(20000)`` and ``synth(5000, 5000)`` by default:

* (a) per metric (jc, peq) and per list length (10^4, 10^6, 10^7 random pairs s < t): ``fill_pairs`` against the same list sent as
  groups of two through ``fill_groups`` -- the only route for named pairs before the pair-list fill --: HIP-event ms
  (pc_stats.ms_total) and wall seconds with the copies, min of ``--steps`` after ``--warmup``; for jc also the sort and the walker
  alone (pc_stats.ms_plan / ms_reduce of a pair-list fill).  A call whose warm-up took longer than ``--slow`` seconds is measured
  once, and the line says so.
* (b) peq edge lists at d <= 0.75, 0.5 and 0.25, plain (``fill_edges``) and behind the af bound (``edges_de_novo(prefilter=True)``'s
  three steps): wall seconds of the call, n_alignments and n_distinct_alignments of both, the candidates, and the PCIe legs of the
  candidate list (the af list's copy to the host, in ms; the candidates' bytes back to the device).

The output file is written anew (``--append``: added to) and flushed line by line, so a run that is cut short still leaves what it
measured."""

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def measured(call, steps, warmup, slow):
    """(min ms_total, min wall seconds, last stats, steps measured) of ``call() -> (result, stats)``."""
    ms, wall, st, seconds = [], [], None, 0.0
    for k in range(warmup + steps):
        if k > warmup and seconds > slow:                 # a slow call: one measured step
            break
        t0 = time.perf_counter()
        _, st = call()
        seconds = time.perf_counter() - t0
        if k >= warmup:
            ms.append(st["ms_total"]); wall.append(seconds)
    return min(ms), min(wall), st, len(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--workloads", nargs="+", default=["real20000", "synth5000"])
    ap.add_argument("--metrics", nargs="+", default=["jc", "peq"])
    ap.add_argument("--lengths", type=int, nargs="+", default=[10 ** 4, 10 ** 6, 10 ** 7])
    ap.add_argument("--groups-above", type=int, default=10 ** 7, help="skip the groups-of-two route for lists longer than this")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.75, 0.5, 0.25])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slow", type=float, default=4.0, help="seconds above which a call is measured once instead of --steps times")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pairs_fill.txt"))
    a = ap.parse_args()
    from phamclust_amd import hip, matrix as M
    from phamclust_amd.results.edges import _prefiltered_peq_edges
    from phamclust_amd.synth import synth_packed, synth_real
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "a" if a.append else "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    try:
        import torch
        device = torch.cuda.get_device_name(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    except Exception:          # noqa: BLE001 -- the name is a label of the record, nothing more
        device = "unnamed device"
    say(f"pair-list fill on one {device}: library version {hip.load().pc_version()}, min of {a.steps} after {a.warmup} warm-up "
        f"(one step where the warm-up took more than {a.slow} s)")
    ctx = M.get_context()
    for workload in a.workloads:
        n = int(workload.lstrip("realsynth"))
        packed = synth_real(n) if workload.startswith("real") else synth_packed(n, n)
        t0 = time.perf_counter()
        ctx.upload(packed, residues=True)
        say(f"{workload}: {packed.n_genomes:,} genomes, {packed.n_pairs:,} pairs; upload {time.perf_counter() - t0:.3f} s")
        rng = np.random.default_rng(packed.n_genomes)
        for length in a.lengths:
            first = rng.integers(0, packed.n_genomes, length)
            second = (first + rng.integers(1, packed.n_genomes, length)) % packed.n_genomes
            s, t = np.minimum(first, second).astype(np.int32), np.maximum(first, second).astype(np.int32)
            groups = np.stack([s, t], axis=1)
            for metric in a.metrics:
                ms, wall, st, taken = measured(lambda: ctx.fill_pairs(metric, s, t, want_stats=True), a.steps, a.warmup, a.slow)
                line = (f"  (a) {metric:>3} {length:>10,} pairs: fill_pairs {ms:10.3f} ms on the device, {wall:8.3f} s with the copies ({taken} step(s))")
                if metric in ("gcs", "jc", "pocp", "af"):
                    line += f"; sort {st['ms_plan']:.3f} ms, walker alone {st['ms_reduce']:.3f} ms"
                else:
                    line += (f"; {st['n_alignments']:,} alignments, {st['n_distinct_alignments']:,} distinct, {st['n_chunks']} chunk(s); plan {st['ms_plan']:.1f}, "
                             f"align {st['ms_align']:.1f}, reduce {st['ms_reduce']:.1f} ms")
                say(line)
                if length <= a.groups_above:
                    g_ms, g_wall, _, g_taken = measured(lambda: ctx.fill_groups(metric, groups, want_stats=True), a.steps, a.warmup, a.slow)
                    say(f"      {'':>3} {'':>10}  as groups of two: {g_ms:10.3f} ms on the device, {g_wall:8.3f} s with the copies ({g_taken} step(s)): "
                        f"{g_ms / max(ms, 1e-9):.2f} x / {g_wall / max(wall, 1e-9):.2f} x the pair-list fill")
        for threshold in a.thresholds:
            plain_ms, plain_wall, plain, _ = measured(lambda: (None, ctx.fill_edges("peq", threshold, want_stats=True, borrow=True)[3]), a.steps, a.warmup, a.slow)
            fast_ms, fast_wall, fast, _ = measured(lambda: (None, _prefiltered_peq_edges(ctx, threshold, True, 0)[3]), a.steps, a.warmup, a.slow)
            say(f"  (b) peq edges at d <= {threshold}: plain {plain_wall:8.3f} s ({plain['n_edges']:,} edges, {plain['n_alignments']:,} alignments, "
                f"{plain['n_distinct_alignments']:,} distinct); prefilter {fast_wall:8.3f} s ({fast['n_edges']:,} edges of {fast['n_candidates']:,} candidates, "
                f"{fast['n_alignments']:,} alignments, {fast['n_distinct_alignments']:,} distinct; af list {fast['af_ms_total']:.3f} ms + {fast['af_ms_d2h']:.3f} ms to the "
                f"host, {8 * fast['n_candidates']:,} bytes back): {plain_wall / max(fast_wall, 1e-9):.2f} x"
                + ("" if fast_wall < plain_wall else "  [prefilter does NOT win here]"))
    out.close()


if __name__ == "__main__":
    main()
