"""Time the affinity fill (pc_fill_affinity) against the only route the commit before it offers: ``python tools/affinity_timing.py``.

One GPU, one process.  Workloads: those of tools/between_timing.py -- jc on synth_real(--n, default 20000) and peq on
synth_real(--n-peq, default 5000), both with the components at d < 0.75 as the groups (cut to the 2,048 largest-first labels when there
are more), plus jc with one group and with 2,048 round-robin labels.  Per workload, ``--repeats`` calls after ``--warmup``, minimum,
median and every value (ms):
  fill       device time of the slabs' fills (pc_stats.ms_total, HIP events)
  rows       device time of k_aff_rows summed over the slabs (pc_last_affinity_times, HIP events), and the bytes of slab per second it
             amounts to (8 bytes per pair)
  cols       the same of k_aff_cols
  finish     device time of k_aff_finish (HIP events)
  call       host clock around Context.fill_affinity(borrow=True), which ends synchronised: only the O(N) arrays cross PCIe
and, alternated with it call by call on the same context:
  dense      host clock around Context.fill(borrow=True): the whole fill and its D2H copy
  ratio      dense / call
``GroupAffinity.from_dense`` on the delivered vector -- the host statement the dense route still needs -- is timed ONCE per workload and
the two results are compared then, exactly.  The output is what profiles/affinity_fill.txt records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  spread {max(xs) - min(xs):8.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=20000, help="genomes of the jc workloads")
    ap.add_argument("--n-peq", type=int, default=5000, help="genomes of the peq workload")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.matrix import GroupAffinity, SymMatrix
    from phamclust_amd.synth import synth_real
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    top = hip.Context.BETWEEN_MAX_GROUPS
    arrays = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")
    say(f"affinity fill against dense fill + D2H (+ host statement): library version {hip.load().pc_version()}, source block "
        f"{hip.Context.affinity_block()}, {a.repeats} calls after {a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    packed_of = {}
    for metric, n, kind in (("jc", a.n, "components"), ("peq", a.n_peq, "components"), ("jc", a.n, "one group"), ("jc", a.n, f"{top} round-robin")):
        if n not in packed_of:
            packed_of[n] = synth_real(n)
        pairs = n * (n - 1) // 2
        ctx.upload(packed_of[n], residues=metric in hip.NEEDS_RESIDUES)
        if kind == "components":
            roots = ctx.fill_components(metric, 0.75)
            _, label = np.unique(roots, return_inverse=True)
            sizes = np.bincount(label)
            rank = np.empty(sizes.shape[0], dtype=np.int64)
            rank[np.argsort(-sizes, kind="stable")] = np.arange(sizes.shape[0])
            label = np.minimum(rank[label], top - 1).astype(np.int32)       # (more components than the limit: the smallest share the last label)
        elif kind == "one group":
            label = np.zeros(n, dtype=np.int32)
        else:
            label = (np.arange(n) % top).astype(np.int32)
        g = int(label.max()) + 1
        say(f"\n{metric} {kind}: synth_real({n}), {pairs:,} pairs, dense vector {pairs * 8 / 1e6:,.1f} MB, {g} groups, resident table "
            f"{hip.Context.affinity_bytes(n, g) / 1e6:,.2f} MB, delivered {n * 44 / 1e6:,.2f} MB")
        got = {key: [] for key in ("fill", "rows", "cols", "finish", "call", "dense")}
        same, host_s = None, 0.0
        for step in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            found = ctx.fill_affinity(metric, label, g, want_stats=True, borrow=True)
            call = time.perf_counter() - t0
            st = found["stats"]
            kept = [np.array(found[name]) for name in arrays]
            t0 = time.perf_counter()
            condensed = ctx.fill(metric, borrow=True)
            dense = time.perf_counter() - t0
            if same is None:
                names = [f"n{k}" for k in range(n)]
                t0 = time.perf_counter()
                order = np.argsort(label, kind="stable")
                cuts = np.searchsorted(label[order], np.arange(g + 1))
                want = GroupAffinity.from_dense(SymMatrix.from_condensed(names, np.asarray(condensed), is_distance=True),
                                                [[names[i] for i in order[cuts[k]:cuts[k + 1]].tolist()] for k in range(g)], want_table=False)
                host_s = time.perf_counter() - t0
                same = all(np.array_equal(x, getattr(want, name)) for x, name in zip(kept, arrays))
                del want
            if step >= a.warmup:
                for key, x in (("fill", st["ms_total"]), ("rows", st["ms_rows"]), ("cols", st["ms_cols"]), ("finish", st["ms_finish"]),
                               ("call", call * 1e3), ("dense", dense * 1e3)):
                    got[key].append(x)

        def rate(key):
            return pairs * 8 / (min(got[key]) * 1e-3) / 1e12 if min(got[key]) > 0 else 0.0

        say(f"  {st['n_slabs']} slab(s); the two routes agree on the result: {same}")
        say(f"    fill (device)         {spread(got['fill'])}")
        say(f"    affinity: rows        {spread(got['rows'])}   = {rate('rows'):.2f} TB/s of slab")
        say(f"    affinity: cols        {spread(got['cols'])}   = {rate('cols'):.2f} TB/s of slab")
        say(f"    affinity: finish      {spread(got['finish'])}")
        say(f"    affinity: call        {spread(got['call'])}")
        say(f"    dense route: fill+D2H {spread(got['dense'])}")
        say(f"    dense route: host statement (GroupAffinity.from_dense, once) {host_s * 1e3:,.1f} ms")
        say(f"    ratio dense / call    min {min(got['dense']) / min(got['call']):.1f}x   median "
            f"{statistics.median(got['dense']) / statistics.median(got['call']):.1f}x   (with the host statement: "
            f"{(min(got['dense']) + host_s * 1e3) / min(got['call']):.1f}x)")
    ctx.close()
    if a.out:
        with open(a.out, "w") as handle:
            handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
