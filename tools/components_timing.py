"""Time the components fill (pc_fill_components) against the route the commit before it offers: ``python tools/components_timing.py``.

One GPU.  Configurations: jc on synth(5000,5000) and synth(20000,5000), peq on synth(5000,5000), each at d < 0.6 and d < 0.75, as
one slab (where the triangle fits the automatic cut this IS the automatic cut, and a second row forces ``--slabs`` slabs) and under
the automatic cut.  Per configuration, ``--steps`` calls after ``--warmup``, every value listed so that the spread shows:
  fill       device time of the slabs' fills (pc_stats.ms_total, HIP events)
  union      device time of the k_cc_union passes (pc_last_component_times, HIP events), against the algorithmic 8 B per pair read
  labels     device time of the k_cc_labels rounds (HIP events)
  wall       host clock around Context.fill_components(borrow=True), which ends synchronised
and, alternated with it call by call in the same process, the previous route to the same labels:
  edges      host clock around Context.fill_edges(borrow=True) at the same threshold (non-strict there: the list's own predicate; its
             device-side compaction and copy times beside it)
  host cc    host clock around SparseEdges.components() over that list (scipy.sparse.csgraph), strict at the threshold
The two label vectors are compared once per configuration.  A last row times the union pass on ``--identical`` identical genomes
(every pair passes, one component: maximal compare-and-swap contention) against the same stream with no pair passing.  The output is what profiles/components_fill.txt records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
CONFIGS = (("jc", 5000), ("jc", 20000), ("peq", 5000))
THRESHOLDS = (0.6, 0.75)


def spread(xs):
    return f"min {min(xs):9.3f}  median {statistics.median(xs):9.3f}  max {max(xs):9.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slabs", type=int, default=4, help="slabs of the forced multi-slab row (slab_bytes = dense bytes / this)")
    ap.add_argument("--identical", type=int, default=5000, help="genomes of the identical-genomes (maximal contention) row")
    ap.add_argument("--configs", default=None, help="comma-separated metric:N pairs instead of the default three")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.matrix import SparseEdges
    from phamclust_amd.synth import synth_packed
    configs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(",")] if a.configs else CONFIGS
    print(f"components fill against edge list + host union-find: library version {hip.load().pc_version()}, {a.steps} calls after {a.warmup} warm-up, ms")
    for metric, n in configs:
        pairs = n * (n - 1) // 2
        packed = synth_packed(n, a.phams)
        ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
        ctx.upload(packed, residues=metric in hip.NEEDS_RESIDUES)
        print(f"\n{metric} synth({n},{a.phams}): {pairs:,} pairs, dense vector {pairs * 8 / 1e6:,.1f} MB, labels {n * 4 / 1e3:,.1f} KB")
        for thr in THRESHOLDS:
            for slab_bytes in (0, max(pairs * 8 // a.slabs, 8)):
                got = {k: [] for k in ("fill", "union", "labels", "wall", "edges", "edges_compact", "edges_d2h", "host_cc")}
                same = None
                for k in range(a.warmup + a.steps):
                    t0 = time.perf_counter()
                    labels, st = ctx.fill_components(metric, thr, slab_bytes=slab_bytes, want_stats=True, borrow=True)
                    wall = (time.perf_counter() - t0) * 1e3
                    labels = np.array(labels)
                    t0 = time.perf_counter()
                    src, tgt, val, est = ctx.fill_edges(metric, thr, slab_bytes=slab_bytes, want_stats=True, borrow=True)
                    t1 = time.perf_counter()
                    host = SparseEdges(range(n), np.asarray(src), np.asarray(tgt), np.asarray(val)).components(thr, strict=True)
                    t2 = time.perf_counter()
                    if same is None:
                        same = bool(np.array_equal(host, labels))
                    if k >= a.warmup:
                        got["fill"].append(st["ms_total"]); got["union"].append(st["ms_union"]); got["labels"].append(st["ms_labels"]); got["wall"].append(wall)
                        got["edges"].append((t1 - t0) * 1e3); got["edges_compact"].append(est["ms_compact"]); got["edges_d2h"].append(est["ms_d2h"])
                        got["host_cc"].append((t2 - t1) * 1e3)
                rate = pairs * 8 / (min(got["union"]) * 1e-3) if min(got["union"]) > 0 else 0.0
                print(f"  d < {thr}, slab_bytes {slab_bytes:,} -> {st['n_slabs']} slab(s): {st['n_edges']:,} pairs pass ({100.0 * st['n_edges'] / pairs:.2f} %), "
                      f"{st['n_components']:,} components; edge list {est['n_edges']:,} edges = {est['n_edges'] * 16 / 1e6:,.1f} MB; labels agree: {same}")
                for key, name in (("fill", "fill (device)"), ("union", "union (device)"), ("labels", "labels (device)"), ("wall", "components wall"),
                                  ("edges", "fill_edges wall"), ("edges_compact", "  its compaction"), ("edges_d2h", "  its edge copy"),
                                  ("host_cc", "host components")):
                    print(f"      {name:<18} {spread(got[key])}")
                print(f"      union: {pairs * 8 / 1e6:,.1f} MB read at {rate / 1e12:.2f} TB/s = {100.0 * rate / HBM_PEAK:.0f} % of the HBM peak; "
                      f"union / one count pass of the edge route (compaction / 2) = {min(got['union']) / max(min(got['edges_compact']) / 2, 1e-9):.2f}; "
                      f"components wall / (fill_edges wall + host components) = {min(got['wall']) / (min(got['edges']) + min(got['host_cc'])):.2f}")
        ctx.close()
    # the most contended union there is: identical genomes, every pair passes and every hook aims at genome 0
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    n = a.identical
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:05d}")
        for j in range(4):
            g.add(f"p{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        genomes.append(g)
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    ctx.upload(pack_genomes(genomes), residues=False)
    pairs = n * (n - 1) // 2
    union, none = [], []
    for k in range(a.warmup + a.steps):
        labels, st = ctx.fill_components("jc", 0.5, want_stats=True)
        assert not labels.any() and st["n_edges"] == pairs
        _, st0 = ctx.fill_components("jc", 0.0, want_stats=True)                  # d < 0: the same stream, no pair passes
        if k >= a.warmup:
            union.append(st["ms_union"]); none.append(st0["ms_union"])
    print(f"\njc, {n} identical genomes: {pairs:,} pairs, all passing, one component")
    print(f"      union, every pair   {spread(union)}")
    print(f"      union, no pair      {spread(none)}")
    print(f"      contention: {min(union) / max(min(none), 1e-9):.1f} x the bare stream, {min(union) * 1e6 / pairs:.2f} ns per passing pair")
    ctx.close()


if __name__ == "__main__":
    main()
