"""Time a rows fill (pc_fill_rows) against the whole fill of the same collection: ``python tools/rows_fill_bench.py``.

One process, one GPU.  synth(N, P) (default 5000, 5000), ``-m peq`` and ``-m jc``, M evenly spaced query rows (default 50 and
500): HIP-event milliseconds (pc_stats.ms_total) of the rows fill, of the whole fill in the same process, the pair share
M(N-1) - M(M-1)/2 over N(N-1)/2, and the measured time beside "pair share x whole fill".  For jc (a set metric: the rows walker
against the selector's tile kernels) a sweep over M gives the first M at which the rows walker stops beating the whole fill.
The output is what profiles/rows_fill.txt records.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(call, warmup, steps):
    for _ in range(warmup):
        call()
    ms = [call()[1]["ms_total"] for _ in range(steps)]
    return min(ms), sum(ms) / len(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--genomes", type=int, default=5000)
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--rows", type=int, nargs="+", default=[50, 500])
    ap.add_argument("--sweep", type=int, nargs="+", default=[25, 50, 100, 200, 350, 500, 750, 1000, 1500, 2500, 5000], help="M values of the jc crossover sweep")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    n = a.genomes
    packed = synth_packed(n, a.phams)
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    ctx.upload(packed)
    whole_pairs = n * (n - 1) // 2
    print(f"rows fill against the whole fill: synth({n},{a.phams}), library version {hip.load().pc_version()}, "
          f"HIP-event ms (pc_stats.ms_total), min / mean of {a.steps} after {a.warmup} warm-up")

    def rows_of(m):
        return np.unique(np.linspace(0, n - 1, m).astype(np.int64))

    whole = {}
    for metric in ("peq", "jc"):
        whole[metric] = timed(lambda: ctx.fill(metric, want_stats=True, borrow=True), a.warmup, a.steps)
        print(f"{metric:>4} whole fill: {whole[metric][0]:9.3f} / {whole[metric][1]:9.3f} ms   ({whole_pairs} pairs)")
    for metric in ("peq", "jc"):
        for m in a.rows:
            rows = rows_of(m)
            m = len(rows)
            _, st = ctx.fill_rows(metric, rows, want_stats=True)
            lo, mean = timed(lambda: ctx.fill_rows(metric, rows, want_stats=True), a.warmup, a.steps)
            share = st["n_pairs"] / whole_pairs
            expect = share * whole[metric][0]
            print(f"{metric:>4} M = {m:5d}: {lo:9.3f} / {mean:9.3f} ms   pair share {100 * share:6.2f} %   share x whole = {expect:8.3f} ms   "
                  f"measured - that = {lo - expect:+8.3f} ms   measured / that = {lo / expect:6.2f}   of the whole fill {100 * lo / whole[metric][0]:6.2f} %   "
                  f"chunks {st['n_chunks']}, plan / align / reduce {st['ms_plan']:.3f} / {st['ms_align']:.3f} / {st['ms_reduce']:.3f} ms")
    crossover = None
    print("  jc sweep (rows walker against the whole fill's kernel, the selector's choice: " + str(ctx.last_set_kernel() or "-") + "):")
    ctx.fill("jc")
    print(f"       whole fill runs on '{ctx.last_set_kernel()}'")
    for m in a.sweep:
        rows = rows_of(min(m, n))
        lo, mean = timed(lambda: ctx.fill_rows("jc", rows, want_stats=True), 1, a.steps)
        print(f"       M = {len(rows):5d}: {lo:8.3f} ms   ({lo / whole['jc'][0]:6.2f} x the whole fill)")
        if crossover is None and lo >= whole["jc"][0]:
            crossover = len(rows)
    print(f"  jc crossover: the rows walker stops beating the whole fill ({whole['jc'][0]:.3f} ms) at M = "
          + (f"{crossover} (first swept M that is not faster)" if crossover else f"none of the swept M up to {max(a.sweep)}"))
    ctx.close()


if __name__ == "__main__":
    main()
