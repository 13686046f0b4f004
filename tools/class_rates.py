#!/usr/bin/env python3
"""Serialised per-class rates of the K4 systolic variants, the record the choosers of pc_nw_shape.hip read.

    python tools/class_rates.py --out profiles/r10/class_rates.json          (on the GPU: measure)
    python tools/class_rates.py --fill-ab label=file.json ... --out ...      (add whole-fill bench lines to the record)
    python tools/class_rates.py --emit-header --out ...                      (no GPU: write phamclust_amd/csrc/pc_nw_rates.h)

One launch class at a time, never two on the chip together: uniform column genes of one length, buckets of `rows` row genes,
the variant forced through pc_align_pairs (1000 + w: the buckets cut as a fill cuts them -- remainder chooser, small-task
modes) and the cell through PC_INC16 (read once: a child process per cell; 2 = the profile cell wherever a workgroup shape
holds its profile, segments of 64 lanes included).  A run is as many calls as sum to 50 ms of kernel time (pc_last_align_ms);
a point is three runs: mean and largest distance from the mean.

Grid: per length every variant whose cost under the model (pc_nw_shape.hip, model_step: the r01-r04 fit) is within 20 % of the
cheapest, plus the chooser's; both cells where compiled and the LDS arithmetic of waves_for allows.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np

LENS = [60, 100, 140, 180, 220, 260, 300, 340, 400, 500, 600, 700, 800, 1000, 1200]
VARIANTS = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 24, 32, 48, 64]
INC16_MAX_W, MAX_SEG, WIN = 24, 16, 32


# ---- host arithmetic of pc_nw_shape.hip, mirrored --------------------------------------------------------------------
def nseg_of(G):
    return min(64 // G, MAX_SEG)


def g_bucket(G):
    return 8 if G <= 8 else 16 if G <= 16 else 32 if G <= 32 else 64


def lds_bytes(W, G, nw, inc16):
    Gb = g_bucket(G)
    rpl = 64 // Gb
    nseg_max = MAX_SEG if Gb == 8 else min(64 // (Gb // 2 + 1), MAX_SEG)
    prof_rows = 25 if inc16 else 24
    row_dwords = (W + 3) // 4 + ((W + 1) // 2 if inc16 else 0)
    lines = 2 * ((prof_rows + 1) // 2) if inc16 and Gb == 64 else (prof_rows + rpl - 1) // rpl
    return (144 + nw * (4 * 64 + 2 * MAX_SEG + nseg_max * WIN)) * 4 + lines * row_dwords * 256


def inc16_fits(W, Gb):
    if W > INC16_MAX_W:
        return False
    nw = 4
    while nw <= (8 if W <= 24 else 4):
        if (160 * 1024 // lds_bytes(W, Gb, nw, True)) * nw >= 16:
            return True
        nw *= 2
    return False


def model_step(W, nseg):
    pen = 1.15 if W >= 64 else 1.08 if W >= 48 else 1.04 if W >= 32 else 1.022 if W >= 24 else 1.014 if W >= 22 else 1.0
    return (W + 0.3 + 0.535 * nseg) * pen


def model_inc16(W, Gb):
    return W <= INC16_MAX_W and ((Gb <= 16 and W <= 22) or (Gb == 32 and 11 <= W <= 19))


def model_cost(L, W):
    G = -(-L // W)
    if G > 64:
        return None
    return model_step(W, nseg_of(G)) * (0.94 if model_inc16(W, g_bucket(G)) else 1.0) / nseg_of(G)


def model_choice(L):
    costs = [(model_cost(L, W), i) for i, W in enumerate(VARIANTS) if model_cost(L, W) is not None]
    return VARIANTS[min(costs)[1]]


def grid(lens, rows_list, common):
    """[(L, rows, W, cell)] -- cell 0 compare, 1 profile"""
    pts = []
    for L in lens:
        best = min(c for c in (model_cost(L, W) for W in VARIANTS) if c is not None)
        ws = [W for W in VARIANTS if model_cost(L, W) is not None and (model_cost(L, W) <= 1.2 * best or W == model_choice(L))]
        for rows in rows_list:
            if rows != 64 and L not in common:
                continue
            for W in ws:
                pts.append((L, rows, W, 0))
                if inc16_fits(W, g_bucket(-(-L // W))):
                    pts.append((L, rows, W, 1))
    return pts


# ---- the measurement (child: one cell) -----------------------------------------------------------------------------
def child(a):
    from phamclust_amd import build, hip
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    build.build_all()
    cell = int(a.child)
    assert os.environ.get("PC_INC16") == ("2" if cell else "0")
    pts = [p for p in grid(a.lens, a.rows, a.common) if p[3] == cell]
    rng = np.random.default_rng(1)
    aa = np.array(list("ACDEFGHIKLMNPQRSTVWY"))
    ctx = hip.Context(0)
    sink = open(a.out, "a")                                   # a line per point as it is taken: a child ended early leaves what it has
    for R in a.rows:                                          # (the 64-row grid first)
        for L in a.lens:
            mine = [p for p in pts if p[0] == L and p[1] == R]
            if not mine:
                continue
            ncols = int(max(64, min(a.max_pairs // R, a.cells / (L * L) / R)))
            g, h = Genome("cols"), Genome("rows")
            for i in range(ncols):
                g.add(f"c{i:05d}", "".join(aa[rng.integers(0, 20, L)]))
            for i in range(R):
                h.add(f"r{i:03d}", "".join(aa[rng.integers(0, 20, max(1, L + int(rng.integers(-L // 20 - 1, L // 20 + 2))))]))
            pk = pack_genomes([g, h])
            ctx.upload(pk)
            rows = np.repeat(np.arange(ncols, ncols + R, dtype=np.int32), ncols)
            cols = np.tile(np.arange(ncols, dtype=np.int32), R)
            lens = np.diff(pk.seq_off)
            cells = float(np.sum(lens[rows].astype(np.float64) * lens[cols]))
            row_res = float(np.sum(lens[rows].astype(np.float64)))
            for _, _, W, _ in mine:
                ctx.align_pairs(rows, cols, variant=W, like_fill=True)               # warm-up
                runs, calls = [], 0
                for _ in range(a.repeats):
                    ms, calls = 0.0, 0
                    while ms < a.min_ms and calls < a.max_calls:
                        ctx.align_pairs(rows, cols, variant=W, like_fill=True)
                        ms += ctx.last_align_ms(); calls += 1
                    runs.append(ms / calls)
                G = -(-L // W)
                mean = sum(runs) / len(runs)
                spread = max(abs(r - mean) for r in runs)
                pt = {"L": L, "rows": R, "W": W, "cell": cell, "G": G, "nseg": nseg_of(G), "waves": hip.Context.task_shape(L, W)["waves"],
                      "columns": ncols, "calls_per_run": calls, "ms_per_call": runs, "gcups": cells / mean / 1e6,
                      # time of one row step of one wave, up to the constant "waves on the chip": kernel time x streams per wave / rows' residues
                      "step_ns": mean * 1e6 * nseg_of(G) / row_res, "step_spread_ns": spread * 1e6 * nseg_of(G) / row_res}
                sink.write(json.dumps(pt) + "\n"); sink.flush()
                print(json.dumps(pt), flush=True)


def kernel_source_hash():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pc_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernel_source_hash()


def measure(a):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    points, incomplete = [], []
    for cell in (0, 1):
        part = a.out + f".cell{cell}"
        env = dict(os.environ, PC_INC16="2" if cell else "0")
        argv = [sys.executable, os.path.abspath(__file__), "--child", str(cell), "--out", part, "--lens", ",".join(map(str, a.lens)),
                "--rows", ",".join(map(str, a.rows)), "--common", ",".join(map(str, a.common)), "--repeats", str(a.repeats),
                "--min-ms", str(a.min_ms), "--max-calls", str(a.max_calls), "--cells", str(a.cells), "--max-pairs", str(a.max_pairs)]
        if os.path.exists(part):
            os.remove(part)
        try:
            subprocess.run(argv, env=env, check=True, timeout=a.child_timeout)
        except subprocess.TimeoutExpired:
            incomplete.append(cell)
        points += [json.loads(line) for line in open(part)] if os.path.exists(part) else []
    rec = {"what": "tools/class_rates.py: serialised per-class step cost of the K4 systolic variants", "kernel_source_hash": kernel_source_hash(),
           "protocol": {"lens": a.lens, "rows": a.rows, "common_lens_for_small_buckets": a.common, "repeats": a.repeats, "min_ms_per_run": a.min_ms,
                        "max_calls_per_run": a.max_calls, "max_pairs_per_call": a.max_pairs,
                        "note": "a run is as many pc_align_pairs calls as sum to min_ms of kernel time (a call is capped at max_pairs alignments: the hook plans on the host)"},
           "cells_cut_short_by_the_time_limit": incomplete, "points": points, "fill_ab": {}, "pins": []}
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"{len(points)} points -> {a.out}")


# ---- whole-fill A/B lines into the record ---------------------------------------------------------------------------
def fill_ab(a):
    rec = json.load(open(a.out))
    for item in a.fill_ab:
        label, path = item.split("=", 1)
        for line in open(path):
            line = line.strip()
            if line.startswith("{") and '"ms_per_step"' in line:
                j = json.loads(line)
                rec["fill_ab"].setdefault(label, []).append({"ms_per_step": j["ms_per_step"], "ms_align": j.get("stage_ms", {}).get("ms_align"),
                                                             "genomes": j["config"]["n_genomes"], "steps": j["steps"]})
    json.dump(rec, open(a.out, "w"), indent=1)


# ---- the header -------------------------------------------------------------------------------------------------------
def table_points(rec):
    """The 64-row points in the model's units: [(W, cell, G, step, spread)], and the constant they were divided by."""
    pts = [p for p in rec["points"] if p["rows"] == 64]
    if not pts:
        return [], 1.0
    k = float(np.median([p["step_ns"] / model_step(p["W"], p["nseg"]) for p in pts]))
    same = {}                                                 # two lengths may give one (W, cell, G): one point, their mean; the spread covers both
    for p in pts:
        same.setdefault((p["W"], p["cell"], p["G"]), []).append((p["step_ns"] / k, p["step_spread_ns"] / k))
    out = []
    for key, v in same.items():
        mean = sum(s for s, _ in v) / len(v)
        out.append(key + (mean, max(max(e for _, e in v), max(abs(s - mean) for s, _ in v))))
    return sorted(out), k


def emit_header(a):
    rec = json.load(open(a.out))
    pts, k = table_points(rec)
    path = os.path.join(REPO, "phamclust_amd", "csrc", "pc_nw_rates.h")
    src = open(path).read()
    head, tail = src.index("// Record:"), src.index("// A point is one launch class")
    what = (f"// Record: {os.path.relpath(os.path.abspath(a.out), REPO)}, taken on device code {rec['kernel_source_hash']} (bench.py's kernel_source_hash):\n"
            f"// {len(pts)} points of 64-row buckets; 1 unit = {k:.4f} ns.\n//\n") if pts else \
           ("// Record: profiles/r10/class_rates.json -- no measurement in it yet: the table is empty and every column gene keeps the\n"
            "// variant and the cell of the model in pc_nw.hip (pc_nw_model_*).\n//\n")
    src = src[:head] + what + src[tail:]
    b0 = src.index("static constexpr PcRatePoint pc_nw_rates[] = {") + len("static constexpr PcRatePoint pc_nw_rates[] = {\n")
    b1 = src.index("    {0, 0, 0, 0.f, 0.f},")
    src = src[:b0] + "".join(f"    {{{W}, {c}, {G}, {s:.4f}f, {e:.4f}f}},\n" for W, c, G, s, e in pts) + src[b1:]
    p0 = src.index("static constexpr int pc_nw_rate_pins[][2] = {") + len("static constexpr int pc_nw_rate_pins[][2] = {                    // [first, last] length\n")
    p1 = src.index("    {0, 0},")
    src = src[:p0] + "".join(f"    {{{p['first']}, {p['last']}}},\n" for p in rec.get("pins", [])) + src[p1:]
    open(path, "w").write(src)
    print(f"{len(pts)} points, {len(rec.get('pins', []))} pinned ranges -> {path}")


if __name__ == "__main__":
    ints = lambda s: [int(x) for x in s.split(",") if x]
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10", "class_rates.json"))
    ap.add_argument("--lens", type=ints, default=LENS)
    ap.add_argument("--rows", type=ints, default=[64, 16])
    ap.add_argument("--common", type=ints, default=[140, 180, 220], help="lengths also measured at the bucket sizes other than 64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-ms", type=float, default=50.0)
    ap.add_argument("--max-calls", type=int, default=3)
    ap.add_argument("--cells", type=float, default=2.2e11, help="DP cells per call (capped by --max-pairs)")
    ap.add_argument("--max-pairs", type=int, default=1000000)
    ap.add_argument("--child-timeout", type=int, default=540)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--fill-ab", nargs="*")
    ap.add_argument("--emit-header", action="store_true")
    ap.add_argument("--list", action="store_true", help="print the grid and stop")
    a = ap.parse_args()
    if a.list:
        g = grid(a.lens, a.rows, a.common)
        for L in a.lens:
            print(L, model_choice(L), sorted({(W, c) for l, r, W, c in g if l == L and r == 64}))
        print(len(g), "points")
    elif a.child is not None:
        child(a)
    elif a.emit_header:
        emit_header(a)
    elif a.fill_ab:
        fill_ab(a)
    else:
        measure(a)
