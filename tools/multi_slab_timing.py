"""Time the edge, component and nearest fills over several devices (pc_multi_fill_*): ``python tools/multi_slab_timing.py``.

Configurations: jc on synth(20000,5000) and peq on synth(5000,5000), each with 1, 2 and 4 contexts (``--worlds``) on the devices
``--ids`` names (default: all on device 0).  Per configuration and call (nearest at k = 16, components at distance < 0.75, edges at
distance <= 0.5), ``--steps`` calls after ``--warmup``; of the last:
  wall       host clock around the call (min and median over the steps), beside the single-context call's on the same upload
  exchange   the slowest device's copy of its state to the root (HIP events; edges: the host copy into the root's arrays)
  merge      the root's merge kernel (k_nn_merge / k_cc_merge; edges have none)
  per device its stretch of targets, the pairs in it, fill ms (pc_stats.ms_total summed over its slabs), DP cells and distinct
             alignments of its fills (aai / peq)
  imbalance  max / mean over the devices of the distinct DP cells (aai / peq) or pairs: what the stretch deal leaves uneven -- it
             balances DP cells per target, and a slab merges duplicate sequence pairs, so the cells actually aligned differ
The results are compared with the single-context call's once per configuration, exactly.  With a device id named twice every line
of the output says REHEARSAL: contexts that share one GPU take turns on it, so the wall times show the route's overhead, never a speed-up.  The
output is what profiles/multi_slab_fill.txt records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = (("jc", 20000), ("peq", 5000))
K, COMPONENTS_AT, EDGES_AT = 16, 0.75, 0.5


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--worlds", default="1,2,4")
    ap.add_argument("--ids", default="0", help="device ids, comma-separated; a world larger than the list repeats the last one")
    ap.add_argument("--configs", default=None, help="comma-separated metric:N pairs instead of the default two")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    configs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(",")] if a.configs else CONFIGS
    ids = [int(x) for x in a.ids.split(",")]
    worlds = [int(x) for x in a.worlds.split(",")]
    devices_of = lambda world: [ids[min(r, len(ids) - 1)] for r in range(world)]       # noqa: E731
    # one context per GPU throughout, or a rehearsal: then EVERY line says so
    tag = "REHEARSAL " if any(len(set(devices_of(w))) < w for w in worlds) else ""
    lines = []

    def say(text):
        line = f"{tag}{text}"
        print(line, flush=True)
        lines.append(line)

    say(f"edge, component and nearest fills over several contexts: library version {hip.load().pc_version()}, {a.steps} calls after "
        f"{a.warmup} warm-up, ms")
    single = hip.Context(ids[0])
    for metric, n in configs:
        packed = synth_packed(n, a.phams)
        residues = metric in hip.NEEDS_RESIDUES
        single.upload(packed, residues=residues)
        calls = (("nearest", lambda c: c.fill_nearest(metric, K, want_stats=True, borrow=True)),
                 ("components", lambda c: c.fill_components(metric, COMPONENTS_AT, want_stats=True, borrow=True)),
                 ("edges", lambda c: c.fill_edges(metric, EDGES_AT, want_stats=True, borrow=True)))
        want, single_wall = {}, {}
        for name, call in calls:
            walls = []
            for step in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                *got, st = call(single)
                if step >= a.warmup:
                    walls.append((time.perf_counter() - t0) * 1e3)
            want[name], single_wall[name] = [np.array(x) for x in got], walls
        say("")
        say(f"{metric} synth({n},{a.phams}): {packed.n_pairs:,} pairs; single-context wall min: " +
            ", ".join(f"{name} {min(single_wall[name]):.3f}" for name, _ in calls))
        for world in worlds:
            devices = devices_of(world)
            with hip.MultiContext(devices) as multi:
                multi.upload(packed, residues=residues)
                say(f"  {world} context(s) on devices {devices}" + (": they share a GPU and take turns on it, no speed-up can show" if len(set(devices)) < world else ""))
                for name, call in calls:
                    walls, same = [], None
                    for step in range(a.warmup + a.steps):
                        t0 = time.perf_counter()
                        *got, st = call(multi)
                        wall = (time.perf_counter() - t0) * 1e3
                        if same is None:
                            same = all(np.array_equal(np.array(g), w) for g, w in zip(got, want[name]))
                        if step >= a.warmup:
                            walls.append(wall)
                    say(f"    {name:<11} wall min {min(walls):10.3f}  median {statistics.median(walls):10.3f}  (single context {min(single_wall[name]):.3f}); "
                        f"exchange {st['ms_exchange']:.3f}, merge {st['ms_merge']:.3f}; {st['n_slabs']} slab(s); equals the single-context result: {same}")
                    per, bounds = st["per_device"], st["stretches"]
                    for r, p in enumerate(per):
                        say(f"      device {r}: targets {bounds[r]:>6}..{bounds[r + 1]:<6} {p['n_pairs']:>12,} pairs  fill {p['ms_total']:10.3f}  "
                            f"cells {p['n_cells']:.3e}  distinct alignments {p['n_distinct_alignments']:,}  distinct cells {p['n_distinct_cells']:.3e}")
                    load = [p["n_distinct_cells"] if residues else p["n_pairs"] for p in per]
                    fills = [p["ms_total"] for p in per]
                    say(f"      imbalance (max / mean): {'distinct cells' if residues else 'pairs'} {max(load) / max(statistics.mean(load), 1e-9):.3f}, "
                        f"fill ms {max(fills) / max(statistics.mean(fills), 1e-9):.3f}")
    single.close()
    if a.out:
        with open(a.out, "w") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
