"""Time the rows form of the between-groups fill (pc_fill_rows_between) against the between-groups fill from scratch:
``python tools/grow_table_timing.py``.

One GPU, one process.  Workloads: peq on synth_real(--n-peq, default 5000) with its components at d < 0.75 as the groups, and jc on
synth_real(--n, default 20000) with those components cut to the --groups (default 800) largest-first labels (the smaller components
share the last label), each with 5 / 50 / 500 new genomes (``--new``) spread evenly over the collection; then, on the jc collection with
the largest count of new genomes, one group (whole waves of one group: the reduction path) and 2,048 round-robin labels (every lane
another group, the largest LDS table).  The seed is the table over the old genomes: the [:G, :G] corner of a from-scratch fill in which
the new genomes share a label of their own, G -- no pair of two old genomes is in any other entry.  Once per workload the grown table
is held to the from-scratch fill's (exactly); with 2,048 labels there is no label to spare, so that seed has the partition's counts and
made-up values (the work is the same) and nothing is compared.  Per workload, call by call alternated with ``Context.fill_between`` from scratch on the same
context -- what a user without the rows form must run --, ``--repeats`` calls after ``--warmup``, minimum, median and every value:
  rows fill   device time of the slabs' rows fills (pc_stats.ms_total, HIP events)
  pass        device time of k_between_qrows over the slabs (pc_last_between_times' ms_reduce, HIP events), and the bytes of slab it
              read per second at its minimum
  fold        device time of k_between_fold (ms_finish)
  call        host clock around Context.fill_rows_between(seed=..., borrow=True), which ends synchronised
  scratch     host clock around Context.fill_between(borrow=True)
  ratio       scratch / call
The output is what profiles/rows_between_fill.txt records."""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=20000, help="genomes of the jc workload")
    ap.add_argument("--n-peq", type=int, default=5000, help="genomes of the peq workload")
    ap.add_argument("--groups", type=int, default=800, help="labels the jc workload's components are cut to")
    ap.add_argument("--new", default="5,50,500", help="comma-separated counts of new genomes")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def workload(ctx, metric, n, label, g, m, title):
        rows = np.unique(np.linspace(0, n - 1, m).astype(np.int64)).astype(np.int32)
        say(f"\n{metric} synth_real({n}), {title}, {rows.shape[0]} new genomes: {rows.shape[0] * n:,} values filled instead of {n * (n - 1) // 2:,} pairs")
        if g < hip.Context.BETWEEN_MAX_GROUPS:
            apart = label.copy()
            apart[rows] = g
            seed = tuple(np.array(arr)[:g, :g].copy() for arr in ctx.fill_between(metric, apart, g + 1))
        else:                                                               # (no label to spare: a seed with the partition's counts and made-up values; the work is the same)
            keep = np.ones(n, dtype=bool)
            keep[rows] = False
            old = np.bincount(label[keep], minlength=g).astype(np.int64)
            count = np.outer(old, old)
            np.fill_diagonal(count, old * (old - 1) // 2)
            full = count > 0
            seed = (count * 500000, count, np.where(full, 0, 2**31 - 1).astype(np.int32), np.where(full, 1000000, -1).astype(np.int32))
        exact = g < hip.Context.BETWEEN_MAX_GROUPS
        got = {key: [] for key in ("fill", "pass", "fold", "call", "scratch")}
        same = None
        for step in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            *grown, st = ctx.fill_rows_between(metric, label, rows, g, seed=seed, want_stats=True, borrow=True)
            call = time.perf_counter() - t0
            kept = [np.array(arr) for arr in grown]
            t0 = time.perf_counter()
            whole = ctx.fill_between(metric, label, g, borrow=True)
            scratch = time.perf_counter() - t0
            if same is None and exact:
                same = all(np.array_equal(mine, np.asarray(ref)) for mine, ref in zip(kept, whole))
            if step >= a.warmup:
                for key, x in (("fill", st["ms_total"]), ("pass", st["ms_reduce"]), ("fold", st["ms_finish"]), ("call", call * 1e3), ("scratch", scratch * 1e3)):
                    got[key].append(x)
        say(f"  {st['n_slabs']} slab(s); the grown table and the from-scratch table agree: {same if exact else 'not compared (the label range is full: a made-up seed)'}")
        for key, text in (("fill", "rows fill (device)"), ("pass", "pass (device)"), ("fold", "fold (device)"), ("call", "call wall"),
                          ("scratch", "from-scratch call wall")):
            say(f"    {text:<24}{spread(got[key])}")
        say(f"    pass reads              {rows.shape[0] * n * 8 / 1e6:,.2f} MB of slab: {rows.shape[0] * n * 8 / (min(got['pass']) * 1e-3) / 1e9:,.1f} GB/s at its minimum")
        say(f"    ratio scratch / call    min {min(got['scratch']) / min(got['call']):.1f}x   median "
            f"{statistics.median(got['scratch']) / statistics.median(got['call']):.1f}x")

    from phamclust_amd.synth import synth_real
    say(f"rows form of the between-groups fill against the between-groups fill from scratch: library version {hip.load().pc_version()}, "
        f"{a.repeats} calls after {a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    news = [int(x) for x in a.new.split(",")]
    for metric, n in (("peq", a.n_peq), ("jc", a.n)):
        ctx.upload(synth_real(n), residues=metric in hip.NEEDS_RESIDUES)
        roots = ctx.fill_components(metric, 0.75)
        _, label = np.unique(roots, return_inverse=True)
        if metric == "jc":
            sizes = np.bincount(label)
            rank = np.empty(sizes.shape[0], dtype=np.int64)
            rank[np.argsort(-sizes, kind="stable")] = np.arange(sizes.shape[0])
            label = np.minimum(rank[label], a.groups - 1)
        label = label.astype(np.int32)
        g = int(label.max()) + 1
        if g >= hip.Context.BETWEEN_MAX_GROUPS:
            say(f"\n{metric} synth_real({n}): {g} components are above the fill's groups; cut to {hip.Context.BETWEEN_MAX_GROUPS - 1}")
            label = np.minimum(label, hip.Context.BETWEEN_MAX_GROUPS - 2).astype(np.int32)
            g = int(label.max()) + 1
        for m in news:
            workload(ctx, metric, n, label, g, m, f"{g} groups")
    n = a.n
    workload(ctx, "jc", n, np.zeros(n, dtype=np.int32), 1, max(news), "one group")
    workload(ctx, "jc", n, (np.arange(n) % hip.Context.BETWEEN_MAX_GROUPS).astype(np.int32), hip.Context.BETWEEN_MAX_GROUPS, max(news), "2,048 round-robin labels")
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
