"""Time the rows forms of the edge-list, components and tree fills against the fills from scratch: ``python tools/rows_slab_timing.py``.

One GPU.  Configurations: jc on synth(20000,5000) and peq on synth(5000,5000); k = 5, 50 and 500 new genomes, scattered evenly over
the name order.  Per configuration the stored results -- edge list, components, tree of the N - k old genomes -- come from fills of
the old genomes alone (their own upload: what a user holds); then, on the upload of all N genomes, ``--steps`` calls after
``--warmup`` of each, min / median and every value:
  de novo    host clock around Context.fill_edges / fill_components / fill_tree: the N (N - 1) / 2 pairs
  extend     host clock around Context.fill_rows_edges / fill_rows_components / fill_rows_tree with the stored result as the seed
             (for the edge list: and the host merge of the stored list with the new one, matrix.merge_edge_lists): k N pairs
  fill       device time of the rows fills of the extend call (pc_stats.ms_total, HIP events)
  pass       device time of the new rows passes of the extend call, summed over its slabs (pc_last_edge_times' compaction,
             pc_last_component_times' union, pc_last_tree_times' rounds; HIP events), the bytes one read of the call's slabs comes to
             (8 k N) and the rate that is -- for the tree per LIVE round, each of which reads the slab once, and for the edge list per
             read, of which compaction makes up to two (count, emit) -- against the HBM peak
The grown result is compared with the de novo one once per configuration, exactly.  The output is what profiles/rows_slab_fills.txt
records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
CONFIGS = (("jc", 20000), ("peq", 5000))
NEW = (5, 50, 500)
THRESHOLD = {"jc": 0.75, "peq": 0.75}


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def _ranges(starts, lengths):
    """The indices of the ranges [starts[i], starts[i] + lengths[i]) laid end to end."""
    import numpy as np
    lengths = np.asarray(lengths, dtype=np.int64)
    ends = np.cumsum(lengths)
    return np.repeat(np.asarray(starts, dtype=np.int64) - (ends - lengths), lengths) + np.arange(int(ends[-1]) if ends.shape[0] else 0, dtype=np.int64)


def packed_subset(packed, keep):
    """The packed form of the genomes ``keep`` (ascending indices) of ``packed``: their genes, the phams re-ranked over those present."""
    import numpy as np
    from phamclust_amd.pack import PackedGenomes
    keep = np.asarray(keep, dtype=np.int64)
    n = int(keep.shape[0])
    counts = np.diff(packed.gene_off)[keep]
    gene_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=gene_off[1:])
    genes = _ranges(packed.gene_off[keep], counts)
    present, gene_pham = np.unique(packed.gene_pham[genes], return_inverse=True)
    gene_pham = gene_pham.astype(np.int32)
    lengths = np.diff(packed.seq_off)[genes]
    seq_off = np.zeros(genes.shape[0] + 1, dtype=np.int64)
    np.cumsum(lengths, out=seq_off[1:])
    residues = packed.residues[_ranges(packed.seq_off[genes], lengths)]
    p = int(present.shape[0])
    w = max(1, (p + 63) // 64)
    gene_genome = np.repeat(np.arange(n, dtype=np.int64), counts)
    bitmap = np.zeros(n * w, dtype=np.uint64)
    np.bitwise_or.at(bitmap, gene_genome * w + (gene_pham >> 6), np.uint64(1) << (gene_pham & 63).astype(np.uint64))
    first = np.ones(genes.shape[0], dtype=bool)
    first[1:] = (gene_pham[1:] != gene_pham[:-1]) | (gene_genome[1:] != gene_genome[:-1])
    return PackedGenomes(names=[packed.names[g] for g in keep.tolist()], pham_names=[packed.pham_names[int(x)] for x in present], n_genomes=n, n_phams=p,
                         words_per_row=w, bitmap=bitmap, nph=np.bincount(gene_genome[first], minlength=n).astype(np.int32),
                         ngen=counts.astype(np.int32), tlen=np.add.reduceat(lengths, gene_off[:-1]).astype(np.int64), gene_off=gene_off,
                         gene_pham=gene_pham, seq_off=seq_off, residues=np.ascontiguousarray(residues)).validate()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default=None, help="comma-separated metric:N pairs instead of the default two")
    ap.add_argument("--new", default=None, help="comma-separated numbers of new genomes instead of 5,50,500")
    a = ap.parse_args()
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.matrix import merge_edge_lists
    from phamclust_amd.synth import synth_packed
    configs = [(c.split(":")[0], int(c.split(":")[1])) for c in a.configs.split(",")] if a.configs else CONFIGS
    news = [int(x) for x in a.new.split(",")] if a.new else NEW
    print(f"rows forms of the edge-list, components and tree fills against the fills from scratch: library version {hip.load().pc_version()}, "
          f"{a.steps} calls after {a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    for metric, n in configs:
        thr = THRESHOLD.get(metric, 0.75)
        packed = synth_packed(n, a.phams)
        residues = metric in hip.NEEDS_RESIDUES
        ctx.upload(packed, residues=residues)
        print(f"\n{metric} synth({n},{a.phams}): {n * (n - 1) // 2:,} pairs; threshold d <= / < {thr}")
        de_novo, whole = {}, {}
        for kind, call in (("edges", lambda: ctx.fill_edges(metric, thr, want_stats=True)), ("components", lambda: ctx.fill_components(metric, thr, want_stats=True)),
                           ("tree", lambda: ctx.fill_tree(metric, want_stats=True))):
            de_novo[kind] = []
            for step in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                got = call()
                if step >= a.warmup:
                    de_novo[kind].append((time.perf_counter() - t0) * 1e3)
            whole[kind] = got
            print(f"  de novo {kind:<11}{spread(de_novo[kind])}")
        for k in news:
            if not 0 < k < n:
                continue
            new = np.unique(np.linspace(0, n - 1, k).round().astype(np.int64))
            old = np.setdiff1d(np.arange(n), new)
            ctx.upload(packed_subset(packed, old), residues=residues)                  # the stored results: fills of the old genomes alone
            e_src, e_tgt, e_val = ctx.fill_edges(metric, thr)
            labels = ctx.fill_components(metric, thr)
            t_src, t_tgt, t_val = ctx.fill_tree(metric)
            ctx.upload(packed, residues=residues)
            old_src, old_tgt = old[e_src], old[e_tgt]                                  # the stored list re-indexed: once, as the stored tree and labels are
            seed_labels = np.arange(n, dtype=np.int32)
            seed_labels[old] = old[labels]
            read = 8.0 * new.shape[0] * n
            print(f"  k = {new.shape[0]} new genomes: {new.shape[0] * (n - 1) - new.shape[0] * (new.shape[0] - 1) // 2:,} pairs, one read of the rows slabs {read / 1e6:,.1f} MB")

            def grow_edges():
                s, t, v, st = ctx.fill_rows_edges(metric, thr, new, want_stats=True)
                return merge_edge_lists((old_src, old_tgt, e_val), (s, t, v)), st, st["ms_compact"], 1

            def grow_components():
                got, st = ctx.fill_rows_components(metric, thr, new, seed_labels=seed_labels, want_stats=True)
                return (got,), st, st["ms_union"], 1

            def grow_tree():
                s, t, v, st = ctx.fill_rows_tree(metric, new, seed=(old[t_src], old[t_tgt], t_val), want_stats=True)
                return (s, t, v), st, st["ms_rounds"], max(st["live_rounds"], 1)

            for kind, call in (("edges", grow_edges), ("components", grow_components), ("tree", grow_tree)):
                wall, fill, passes = [], [], []
                for step in range(a.warmup + a.steps):
                    t0 = time.perf_counter()
                    got, st, ms_pass, reads = call()
                    if step >= a.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                        fill.append(st["ms_total"])
                        passes.append(ms_pass)
                same = all(np.array_equal(x, y) for x, y in zip(got, whole[kind][:len(got)] if kind != "components" else (whole[kind][0],)))
                per_read = min(passes) / reads
                print(f"    {kind:<11} the grown result equals the de novo one: {same}; {st['n_slabs']} slab(s)")
                print(f"      extend wall     {spread(wall)}   de novo / extend: {min(de_novo[kind]) / min(wall):.1f}x")
                print(f"      rows fill       {spread(fill)}")
                print(f"      rows pass       {spread(passes)}   {reads} read(s) of {read / 1e6:,.1f} MB: {per_read:.4f} ms each = "
                      f"{read / (per_read * 1e-3) / 1e9:,.1f} GB/s, {100.0 * read / (per_read * 1e-3) / HBM_PEAK:.2f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak")
    ctx.close()


if __name__ == "__main__":
    main()
