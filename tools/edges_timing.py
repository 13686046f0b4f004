"""Time the edge-list fill (pc_fill_edges) against the dense delivery it replaces: ``python tools/edges_timing.py --baseline-lib LIB``.

One GPU.  Configurations: jc on synth(5000,5000) and synth(20000,5000), peq on synth(2000,5000), each at d <= 0.999999 (every
non-zero similarity) and d <= 0.75.  Per configuration, min / median of ``--steps`` calls after ``--warmup``:
  fill      device time of the slabs' fills (pc_stats.ms_total, HIP events)
  compact   device time of count + scan + emit (pc_last_edge_times, HIP events)
  d2h       device time of the edges' copy to the host (HIP events)
  wall      host clock around Context.fill_edges(borrow=True), which ends synchronised
  dense     host clock around pc_fill_borrow of the same collection on ANOTHER library -- ``--baseline-lib``: the build of the commit
            this feature was added to -- in a child process of its own, run before and after the edge-list calls.  That is the
            comparison: the dense delivery as it was, never the new library against itself.
The compaction is an HBM stream: its algorithmic bytes are 2 x 8 B per pair read (count, emit) plus 16 B per edge written, quoted
over ``compact`` as a rate and as a share of the 8.0 TB/s HBM3E peak (6.3 TB/s is what a copy kernel reaches on this part).
The output is what profiles/edges_fill.txt records.
"""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
CONFIGS = (("jc", 5000), ("jc", 20000), ("peq", 2000))
THRESHOLDS = (0.999999, 0.75)


def dense_child(lib_path, metric, n, phams, warmup, steps):
    """In a process of its own: wall time of pc_fill_borrow on ``lib_path`` through a binding of the four calls it needs (an older
    library lacks exports the package's binding declares)."""
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    lib = ctypes.CDLL(lib_path)
    lib.pc_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p

    def check(rc):
        if rc != 0:
            raise SystemExit(f"{lib_path}: status {rc}: {lib.pc_last_error().decode()}")

    packed = synth_packed(n, phams)
    s = hip.Context._struct(packed)
    h = vp()
    lib.pc_ctx_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.pc_upload.argtypes = lib.pc_upload_sets.argtypes = [vp, ctypes.POINTER(hip.PcPacked)]
    lib.pc_fill_borrow.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.POINTER(ctypes.c_double)), ctypes.POINTER(hip.PcStats)]
    lib.pc_ctx_destroy.argtypes = [vp]
    lib.pc_ctx_destroy.restype = None
    check(lib.pc_ctx_create(ctypes.byref(h), int(os.environ.get("PHAMCLUST_DEVICE", "0"))))
    check((lib.pc_upload if metric in hip.NEEDS_RESIDUES else lib.pc_upload_sets)(h, ctypes.byref(s)))
    walls, devs = [], []
    for k in range(warmup + steps):
        ptr, st = ctypes.POINTER(ctypes.c_double)(), hip.PcStats()
        t0 = time.perf_counter()
        check(lib.pc_fill_borrow(h, hip.METRIC_IDS[metric], 1, ctypes.byref(ptr), ctypes.byref(st)))
        wall = (time.perf_counter() - t0) * 1e3
        if k >= warmup:
            walls.append(wall)
            devs.append(st.ms_total)
    lib.pc_version.restype = ctypes.c_int
    version = lib.pc_version()
    lib.pc_ctx_destroy(h)
    print(json.dumps({"version": version, "wall_ms": walls, "device_ms": devs}))


def run_dense_child(a, metric, n):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", metric, str(n), "--baseline-lib", a.baseline_lib, "--phams", str(a.phams),
           "--steps", str(a.steps), "--warmup", str(a.warmup)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if proc.returncode != 0:
        raise SystemExit(f"dense baseline failed ({proc.returncode}): {proc.stdout[-500:]} {proc.stderr[-2000:]}")
    return json.loads(proc.stdout.strip().splitlines()[-1])


def lo_med(xs):
    return f"{min(xs):9.3f} / {statistics.median(xs):9.3f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--baseline-lib", required=True, help="libphamclust_hip.so of the commit before pc_fill_edges (the dense delivery to compare with)")
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", nargs=2, metavar=("METRIC", "N"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.baseline_lib = os.path.abspath(a.baseline_lib)
    if a.child:
        return dense_child(a.baseline_lib, a.child[0], int(a.child[1]), a.phams, a.warmup, a.steps)
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    print(f"edge-list fill against the dense delivery: library version {hip.load().pc_version()}, min / median of {a.steps} after {a.warmup} warm-up, ms")
    for metric, n in CONFIGS:
        pairs = n * (n - 1) // 2
        before = run_dense_child(a, metric, n)
        ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
        ctx.upload(synth_packed(n, a.phams), residues=metric in hip.NEEDS_RESIDUES)
        rows = []
        for thr in THRESHOLDS:
            got = {"fill": [], "compact": [], "d2h": [], "wall": []}
            for k in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                src, tgt, val, st = ctx.fill_edges(metric, thr, want_stats=True, borrow=True)
                wall = (time.perf_counter() - t0) * 1e3
                if k >= a.warmup:
                    got["fill"].append(st["ms_total"]); got["compact"].append(st["ms_compact"]); got["d2h"].append(st["ms_d2h"]); got["wall"].append(wall)
            rows.append((thr, st, got))
        ctx.close()
        after = run_dense_child(a, metric, n)
        dense_wall = before["wall_ms"] + after["wall_ms"]
        print(f"\n{metric} synth({n},{a.phams}): {pairs:,} pairs, dense vector {pairs * 8 / 1e6:,.1f} MB")
        print(f"  dense delivery, pc_fill_borrow on the baseline library (version {before['version']}): wall {lo_med(dense_wall)}   "
              f"(before {lo_med(before['wall_ms'])}, after {lo_med(after['wall_ms'])}; its fill on the device {lo_med(before['device_ms'] + after['device_ms'])})")
        for thr, st, got in rows:
            e = st["n_edges"]
            stream = 2 * 8 * pairs + 16 * e
            rate = stream / (min(got["compact"]) * 1e-3) if min(got["compact"]) > 0 else 0.0
            print(f"  d <= {thr:<8}: {e:>13,} edges = {100.0 * e / pairs:6.2f} % of the pairs, {e * 16 / 1e6:>9,.1f} MB ({e * 16 / (pairs * 8):5.2f} x the dense vector), "
                  f"{st['n_slabs']} slab(s)")
            print(f"      fill {lo_med(got['fill'])}   compact {lo_med(got['compact'])}   d2h {lo_med(got['d2h'])}   wall {lo_med(got['wall'])}")
            print(f"      compaction: {stream / 1e6:,.1f} MB of algorithmic traffic at {rate / 1e12:.2f} TB/s = {100.0 * rate / HBM_PEAK:.0f} % of the HBM peak; "
                  f"wall / dense wall = {min(got['wall']) / min(dense_wall):.2f}")


if __name__ == "__main__":
    main()
