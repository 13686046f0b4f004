"""Time the nearest fill under peq behind its af bound: ``python tools/nearest_bound_timing.py`` writes ``profiles/nearest_bound_fill.txt``.

One process, one GPU, one build.  Per workload -- ``synth(5000, 5000)`` and ``synth_real(5000)`` by default, ``real20000`` on request --
and per K (4, 16, 64): the parent route, ``fill_nearest("peq", K)``, against ``_bounded_peq_nearest`` (``neighbors_de_novo(bound=True)``'s
five steps) call by call, wall seconds, min of ``--steps`` after ``--warmup``.  Per line: candidates / pairs, alignments (seed + final) /
the plain fill's, the host seconds of the steps of the fastest bounded call (seed af lists, seed peq values, seed lists and bars,
candidate pass, final peq values, final lists -- or the plain fill after a fallback), the bytes the pair lists moved over PCIe with the
time like-sized copies take on this machine (pageable host memory, through torch) and its share of the call, and whether the route
fell back.  The lists are compared with the plain fill's on every measured step.

The output file is written anew (``--append``: added to) and flushed line by line, so a run that is cut short still leaves what it
measured."""

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def copy_seconds(n_bytes, device):
    """(up, down): min of 3 of a pageable host -> device and a device -> host copy of ``n_bytes``."""
    import torch
    host = torch.from_numpy(np.zeros(max(n_bytes // 8, 1), dtype=np.float64))
    up, down = [], []
    for _ in range(3):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        there = host.to(device)
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        there.cpu()
        t2 = time.perf_counter()
        up.append(t1 - t0); down.append(t2 - t1)
    return min(up), min(down)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--workloads", nargs="+", default=["synth5000", "real5000"])
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slow", type=float, default=4.0, help="seconds above which a call is measured once instead of --steps times")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nearest_bound_fill.txt"))
    a = ap.parse_args()
    from phamclust_amd import hip, matrix as M
    from phamclust_amd.results.neighbors import _bounded_peq_nearest
    from phamclust_amd.synth import synth_packed, synth_real
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "a" if a.append else "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ordinal = int(os.environ.get("PHAMCLUST_DEVICE", "0"))
    try:
        import torch
        device = torch.cuda.get_device_name(ordinal)
    except Exception:          # noqa: BLE001 -- the name is a label of the record, nothing more
        device = "unnamed device"
    say(f"nearest fill under peq behind the af bound on one {device}: library version {hip.load().pc_version()}, min of {a.steps} after {a.warmup} "
        f"warm-up (one step where the warm-up took more than {a.slow} s), plain and bounded calls alternating on one build")
    ctx = M.get_context()
    for workload in a.workloads:
        n = int(workload.lstrip("realsynth"))
        packed = synth_real(n) if workload.startswith("real") else synth_packed(n, n)
        t0 = time.perf_counter()
        ctx.upload(packed, residues=True)
        say(f"{workload}: {packed.n_genomes:,} genomes, {packed.n_pairs:,} pairs; upload {time.perf_counter() - t0:.3f} s")
        for k in a.ks:
            plain_wall, fast_wall, plain, fast, same, seconds = [], [], None, None, True, 0.0
            for step in range(a.warmup + a.steps):
                if step > a.warmup and seconds > a.slow:
                    break
                t0 = time.perf_counter()
                p_nbr, p_val, plain = ctx.fill_nearest("peq", k, want_stats=True)
                t1 = time.perf_counter()
                f_nbr, f_val, st = _bounded_peq_nearest(ctx, k, True, 0)
                t2 = time.perf_counter()
                seconds = max(t1 - t0, t2 - t1)
                same = same and np.array_equal(p_nbr, f_nbr) and np.array_equal(p_val.view(np.uint64), f_val.view(np.uint64))
                if step >= a.warmup:
                    plain_wall.append(t1 - t0)
                    if not fast_wall or t2 - t1 < min(fast_wall):
                        fast = st
                    fast_wall.append(t2 - t1)
            p, f = min(plain_wall), min(fast_wall)
            up, down = copy_seconds(8 * max(fast["n_candidates"], 1), f"cuda:{ordinal}")
            pcie = 3 * (up + down)                       # per candidate: 16 B down, 8 B up, 8 B down, 16 B up
            steps = " / ".join(f"{x * 1e3:.1f}" for x in fast["step_s"])
            say(f"  K = {k:>2}: plain {p:8.3f} s ({plain['n_alignments']:,} alignments, selection {plain.get('ms_select', 0.0):.1f} ms); bounded {f:8.3f} s "
                f"({len(fast_wall)} step(s)): {fast['n_candidates']:,} candidates of {packed.n_pairs:,} pairs ({100.0 * fast['n_candidates'] / packed.n_pairs:.2f} %), "
                f"{fast['n_seed_pairs']:,} seed pairs, {fast['n_alignments']:,} alignments (seed + final"
                f"{' + the plain fill' if fast['fallback'] else ''}; {100.0 * fast['n_alignments'] / max(plain['n_alignments'], 1):.1f} % of plain), "
                f"{fast['n_distinct_alignments']:,} distinct in the last peq call against {plain['n_distinct_alignments']:,}; steps {steps} ms "
                f"(af fills on the device {fast['af_ms_total']:.1f} ms, candidates to the host {fast['af_ms_d2h']:.2f} ms); lists over PCIe "
                f"{fast['n_list_bytes']:,} bytes, like-sized copies {pcie * 1e3:.2f} ms = {100.0 * pcie / f:.1f} % of the call; "
                f"fallback {fast['fallback']}; same lists: {same}: {p / max(f, 1e-9):.2f} x"
                + ("" if f < p else "  [the bound does NOT win here]"))
    out.close()


if __name__ == "__main__":
    main()
