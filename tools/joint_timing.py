"""Time the joint fill (pc_fill_joint, pc_fill_pairs_joint) against the single fills: ``python tools/joint_timing.py`` writes
``profiles/joint_fill.txt``.

One process, one GPU, one build.  Per workload -- ``synth(5000, 5000)`` and ``synth_real(5000)`` by default:

* (a) the whole triangle: the joint fill of all six metrics, the joint fill of {af, aai, peq}, the peq fill alone, the aai fill alone,
  and the six single fills in sequence;
* (b) ``--pairs`` random pairs s < t (10^6): ``fill_pairs_joint`` of all six metrics against six ``fill_pairs``, and the peq list alone.

Each as device time (pc_stats.ms_total, and ms_reduce: the walk that writes the values) and as the wall time of the call with its
copies to the host.  The calls ALTERNATE -- every round runs each of them once, in the order listed -- and the figure is the minimum over
``--steps`` rounds after ``--warmup`` rounds.  The last lines of a workload state the joint call against the peq fill alone and
against what it replaces.  The output file is written anew and flushed line by line."""

import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SIX = ["gcs", "jc", "pocp", "af", "aai", "peq"]


def alternating(calls, steps, warmup):
    """``calls``: {label: call() -> list of stats dicts, one per library call it made}.  Every round runs each call once, in order;
    returns {label: (min device ms, min reduce ms, min wall s, last stats list)} over the ``steps`` rounds after ``warmup``."""
    seen = {label: ([], [], []) for label in calls}
    last = {}
    for k in range(warmup + steps):
        for label, call in calls.items():
            t0 = time.perf_counter()
            stats = call()
            wall = time.perf_counter() - t0
            last[label] = stats
            if k >= warmup:
                ms, reduce, walls = seen[label]
                ms.append(sum(st["ms_total"] for st in stats)); reduce.append(sum(st["ms_reduce"] for st in stats)); walls.append(wall)
    return {label: (min(ms), min(reduce), min(walls), last[label]) for label, (ms, reduce, walls) in seen.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--workloads", nargs="+", default=["synth5000", "real5000"])
    ap.add_argument("--pairs", type=int, default=10 ** 6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "joint_fill.txt"))
    a = ap.parse_args()
    from phamclust_amd import hip, matrix as M
    from phamclust_amd.synth import synth_packed, synth_real
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "w")

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    try:
        import torch
        device = torch.cuda.get_device_name(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    except Exception:          # noqa: BLE001 -- the name is a label of the record, nothing more
        device = "unnamed device"
    say(f"joint fill on one {device}: library version {hip.load().pc_version()}, calls alternating, min of {a.steps} rounds after {a.warmup} warm-up")
    ctx = M.get_context()

    def report(title, got, order):
        for label in order:
            ms, reduce, wall, stats = got[label]
            st = stats[-1]
            say(f"  {title} {label:<34} {ms:10.3f} ms on the device (walk {reduce:8.3f} ms), {wall:8.3f} s with the copies; "
                f"{st['n_alignments']:,} alignments, {st['n_distinct_alignments']:,} distinct, {st['n_chunks']} chunk(s), {len(stats)} call(s)")

    def against(title, got, joint, peq, replaced):
        j_ms, j_reduce, j_wall, _ = got[joint]
        p_ms, p_reduce, p_wall, _ = got[peq]
        r_ms, _, r_wall, _ = got[replaced]
        say(f"  {title} {joint} / {peq}: {j_ms / max(p_ms, 1e-9):.4f} x on the device ({j_ms - p_ms:+.3f} ms, of which the walk "
            f"{j_reduce - p_reduce:+.3f} ms), {j_wall / max(p_wall, 1e-9):.2f} x with the copies")
        say(f"  {title} {replaced} / {joint}: {r_ms / max(j_ms, 1e-9):.3f} x on the device, {r_wall / max(j_wall, 1e-9):.3f} x with the copies")

    for workload in a.workloads:
        n = int(workload.lstrip("realsynth"))
        packed = synth_real(n) if workload.startswith("real") else synth_packed(n, n)
        t0 = time.perf_counter()
        ctx.upload(packed, residues=True)
        say(f"{workload}: {packed.n_genomes:,} genomes, {packed.n_pairs:,} pairs; upload {time.perf_counter() - t0:.3f} s")
        whole = {
            "joint fill, six metrics": lambda: [ctx.fill_joint(SIX, want_stats=True)[1]],
            "joint fill, af + aai + peq": lambda: [ctx.fill_joint(["af", "aai", "peq"], want_stats=True)[1]],
            "peq fill alone": lambda: [ctx.fill("peq", want_stats=True)[1]],
            "aai fill alone": lambda: [ctx.fill("aai", want_stats=True)[1]],
            "six single fills in sequence": lambda: [ctx.fill(metric, want_stats=True)[1] for metric in SIX],
        }
        got = alternating(whole, a.steps, a.warmup)
        report("(a)", got, list(whole))
        against("(a)", got, "joint fill, six metrics", "peq fill alone", "six single fills in sequence")
        against("(a)", got, "joint fill, af + aai + peq", "peq fill alone", "six single fills in sequence")
        rng = np.random.default_rng(packed.n_genomes)
        first = rng.integers(0, packed.n_genomes, a.pairs)
        second = (first + rng.integers(1, packed.n_genomes, a.pairs)) % packed.n_genomes
        s, t = np.minimum(first, second).astype(np.int32), np.maximum(first, second).astype(np.int32)
        listed = {
            "fill_pairs_joint, six metrics": lambda: [ctx.fill_pairs_joint(SIX, s, t, want_stats=True)[1]],
            "fill_pairs peq alone": lambda: [ctx.fill_pairs("peq", s, t, want_stats=True)[1]],
            "six fill_pairs in sequence": lambda: [ctx.fill_pairs(metric, s, t, want_stats=True)[1] for metric in SIX],
        }
        got = alternating(listed, a.steps, a.warmup)
        title = f"(b) {a.pairs:,} pairs:"
        report(title, got, list(listed))
        against(title, got, "fill_pairs_joint, six metrics", "fill_pairs peq alone", "six fill_pairs in sequence")
    out.close()


if __name__ == "__main__":
    main()
