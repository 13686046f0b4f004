"""Time the tree fill (pc_fill_tree) against the route the commit before it offers: ``python tools/tree_timing.py``.

One GPU.  Configurations: jc on synth(20000,5000) and peq on synth(5000,5000), under the automatic slab cut (and, with ``--slabs S``,
once more cut into S slabs).  Per configuration, ``--steps`` calls after ``--warmup``, min / median and every value:
  fill       device time of the slabs' fills (pc_stats.ms_total, HIP events)
  rounds     device time of the Boruvka rounds summed over the slabs (pc_last_tree_times, HIP events), with the rounds that did work
             and the rounds enqueued (pc_last_tree_rounds), and what one live round comes to against a single read of its slab
  finish     the copy of the N - 1 keys, their sort and their decoding (host clock)
  wall       host clock around Context.fill_tree(borrow=True), which ends synchronised
and, alternated with it call by call on the same context, the only route the commit before offers to the same dendrogram:
  dense      host clock around Context.fill(borrow=True) -- the whole fill and its D2H copy -- plus
             scipy.cluster.hierarchy.linkage(condensed, 'single') on the host
  ratio      dense wall / call wall
The two results are compared once per configuration: the merge heights, exactly.  The output is what profiles/tree_fill.txt records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
CONFIGS = (("jc", 20000), ("peq", 5000))


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def dense_route(ctx, metric):
    """The parent commit's route: whole fill + D2H, then scipy's single linkage.  Returns (heights, seconds of the fill and copy,
    seconds of the host linkage)."""
    import numpy as np
    from scipy.cluster.hierarchy import linkage
    t0 = time.perf_counter()
    condensed = ctx.fill(metric, borrow=True)
    t1 = time.perf_counter()
    z = linkage(np.asarray(condensed), "single")
    t2 = time.perf_counter()
    return z[:, 2].copy(), t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slabs", type=int, default=0, help="also time the call cut into this many slabs (slab_bytes = dense bytes / this)")
    ap.add_argument("--configs", default=None, help="comma-separated metric:N pairs instead of the default two")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    configs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(",")] if a.configs else CONFIGS
    print(f"tree fill against dense fill + host single linkage: library version {hip.load().pc_version()}, {a.steps} calls after "
          f"{a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    for metric, n in configs:
        pairs = n * (n - 1) // 2
        ctx.upload(synth_packed(n, a.phams), residues=metric in hip.NEEDS_RESIDUES)
        print(f"\n{metric} synth({n},{a.phams}): {pairs:,} pairs, dense vector {pairs * 8 / 1e6:,.1f} MB, result {(n - 1) * 16 / 1e6:,.2f} MB")
        for slab_bytes in (0,) + ((max(pairs * 8 // a.slabs, 8),) if a.slabs > 1 else ()):
            got = {key: [] for key in ("fill", "rounds", "finish", "wall", "dense", "dense_fill", "dense_linkage")}
            same = None
            for step in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                src, tgt, val, st = ctx.fill_tree(metric, slab_bytes=slab_bytes, want_stats=True, borrow=True)
                wall = time.perf_counter() - t0
                val = np.array(val)
                heights, fill_s, link_s = dense_route(ctx, metric)
                if same is None:
                    same = bool(np.array_equal(val, heights))
                if step >= a.warmup:
                    for key, x in (("fill", st["ms_total"]), ("rounds", st["ms_rounds"]), ("finish", st["ms_finish"]), ("wall", wall * 1e3),
                                   ("dense", (fill_s + link_s) * 1e3), ("dense_fill", fill_s * 1e3), ("dense_linkage", link_s * 1e3)):
                        got[key].append(x)
            live, launched = st["live_rounds"], st["launched_rounds"]
            per_round = min(got["rounds"]) / max(live, 1)
            read = pairs * 8 / max(st["n_slabs"], 1)                  # a round reads its own slab (about equal ones)
            print(f"  slab_bytes {slab_bytes:,} ({st['n_slabs']} slab(s)); rounds: {live} did work of {launched} enqueued; the two routes agree on the heights: {same}")
            for key, title in (("fill", "fill (device)"), ("rounds", "rounds (device)"), ("finish", "finish (host)"), ("wall", "call wall"),
                               ("dense", "dense route wall"), ("dense_fill", "  its fill + D2H"), ("dense_linkage", "  its host linkage")):
                print(f"    {title:<22}{spread(got[key])}")
            print(f"    ratio dense / call    min {min(got['dense']) / min(got['wall']):.1f}x   median "
                  f"{statistics.median(got['dense']) / statistics.median(got['wall']):.1f}x")
            print(f"    per live round        {per_round:.3f} ms for one read of a slab of {read / 1e9:.3f} GB = {read / (per_round * 1e-3) / 1e12:.2f} TB/s, "
                  f"{100.0 * read / (per_round * 1e-3) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak")
    ctx.close()


if __name__ == "__main__":
    main()
