"""Time the nearest-neighbours fill (pc_fill_nearest) against the route the commit before it offers: ``python tools/nearest_timing.py``.

One GPU.  Configurations: jc on synth(20000,5000) at k = 16 and k = 64, peq on synth(5000,5000) at k = 16, under the automatic slab
cut (and, with ``--slabs S``, once more cut into S slabs).  Per configuration, ``--steps`` calls after ``--warmup``, min / median and
every value:
  fill       device time of the slabs' fills (pc_stats.ms_total, HIP events)
  select     device time of the row and column passes (pc_last_nearest_times, HIP events), against the floor of the design: both
             passes read every slab once, 2 x 8 x Lp bytes (percentage of the HBM peak of 8 TB/s beside it)
  finish     device time of the finishing pass
  wall       host clock around Context.fill_nearest(borrow=True), which ends synchronised
and, alternated with it call by call on the same context, the only route the commit before offers to the same lists:
  dense      host clock around Context.fill(borrow=True) -- the whole fill and its D2H copy -- plus, per row of the square matrix, an
             np.partition at the k-th smallest and a lexsort of those (ties at the k-th place resolved by index: every value equal
             to the k-th is kept for the sort), i.e. NearestNeighbors.from_dense's result without sorting whole rows
  ratio      dense wall / call wall
The two results are compared once per configuration (indices and values, exactly).  The output is what profiles/nearest_fill.txt
records.

``--rows`` times the rows form instead (pc_fill_rows_nearest: stored lists grown by new genomes): jc on synth(20000,5000) and peq on
synth(5000,5000) at k = 16, with 5 / 50 / 500 new genomes (``--new``), spread evenly over the collection.  The stored lists of the old
genomes come from one dense fill and a host selection restricted to them (not timed).  Per configuration, call by call alternated with
``Context.fill_nearest`` from scratch at the same N and k -- what a user without the rows form must run -- ``--steps`` calls after
``--warmup``:
  fill / select / finish / wall   as above, of Context.fill_rows_nearest(borrow=True); select is the two rows passes' own time
  scratch                         host clock around Context.fill_nearest(borrow=True)
  ratio                           scratch wall / grown wall
The grown lists are compared with the from-scratch ones once per configuration (exactly).  The output is what
profiles/rows_nearest_fill.txt records.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12
CONFIGS = (("jc", 20000, 16), ("jc", 20000, 64), ("peq", 5000, 16))
ROWS_CONFIGS = (("jc", 20000, 16), ("peq", 5000, 16))


def spread(xs):
    return f"min {min(xs):10.3f}  median {statistics.median(xs):10.3f}  [{' '.join(f'{x:.3f}' for x in xs)}]"


def dense_route(ctx, metric, n, k):
    """The parent commit's route: whole fill + D2H, then per row partition + sort.  Returns (indices, weights, seconds of the fill
    and copy, seconds of the host selection)."""
    import numpy as np
    from scipy.spatial.distance import squareform
    t0 = time.perf_counter()
    condensed = ctx.fill(metric, borrow=True)
    t1 = time.perf_counter()
    square = squareform(np.asarray(condensed))
    np.fill_diagonal(square, np.inf)                                # a genome is not its own neighbour
    kk = min(k, n - 1)
    nbr = np.empty((n, kk), dtype=np.int32)
    val = np.empty((n, kk), dtype=np.float64)
    for g in range(n):
        row = square[g]
        bar = np.partition(row, kk - 1)[kk - 1]
        cand = np.flatnonzero(row <= bar)                           # the k best and every tie of the k-th
        order = cand[np.lexsort((cand, row[cand]))][:kk]
        nbr[g] = order
        val[g] = row[order]
    t2 = time.perf_counter()
    return nbr, val, t1 - t0, t2 - t1


def stored_lists(square, new, k):
    """The k best old neighbours of every old genome from the square matrix (diagonal inf), as [n, k] seed arrays in the grown
    numbering: the lists a fill of the old genomes alone would have stored."""
    import numpy as np
    n = square.shape[0]
    is_new = np.zeros(n, dtype=bool)
    is_new[new] = True
    old = np.flatnonzero(~is_new)
    ks = min(k, old.shape[0] - 1)
    nbr = np.zeros((n, ks), dtype=np.int32)
    val = np.zeros((n, ks), dtype=np.float64)
    for g in old.tolist():
        row = square[g, old]
        bar = np.partition(row, ks - 1)[ks - 1]
        cand = np.flatnonzero(row <= bar)
        order = cand[np.lexsort((old[cand], row[cand]))][:ks]
        nbr[g] = old[order]
        val[g] = row[order]
    return nbr, val


def rows_mode(a):
    import numpy as np
    from scipy.spatial.distance import squareform
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    configs = [(c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in a.configs.split(",")] if a.configs else ROWS_CONFIGS
    counts = [int(x) for x in a.new.split(",")]
    print(f"rows form of the nearest-neighbours fill against the fill from scratch: library version {hip.load().pc_version()}, {a.steps} calls "
          f"after {a.warmup} warm-up, ms")
    ctx = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    for metric, n, k in configs:
        ctx.upload(synth_packed(n, a.phams), residues=metric in hip.NEEDS_RESIDUES)
        square = squareform(np.asarray(ctx.fill(metric, borrow=True)))
        np.fill_diagonal(square, np.inf)
        for m in counts:
            new = np.unique(np.linspace(0, n - 1, m).astype(np.int64))
            seed = stored_lists(square, new, k)
            print(f"\n{metric} synth({n},{a.phams}) k = {k}, {new.shape[0]} new genomes: {new.shape[0] * n:,} values filled instead of {n * (n - 1) // 2:,} pairs")
            got = {key: [] for key in ("fill", "select", "finish", "wall", "scratch", "scratch_select")}
            same = None
            for step in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                nbr, val, st = ctx.fill_rows_nearest(metric, k, new, seed=seed, want_stats=True, borrow=True)
                wall = time.perf_counter() - t0
                nbr, val = np.array(nbr), np.array(val)
                t0 = time.perf_counter()
                w_nbr, w_val, w_st = ctx.fill_nearest(metric, k, want_stats=True, borrow=True)
                scratch = time.perf_counter() - t0
                if same is None:
                    same = bool(np.array_equal(nbr, w_nbr) and np.array_equal(val.view(np.uint64), np.asarray(w_val).view(np.uint64)))
                if step >= a.warmup:
                    for key, x in (("fill", st["ms_total"]), ("select", st["ms_select"]), ("finish", st["ms_finish"]), ("wall", wall * 1e3),
                                   ("scratch", scratch * 1e3), ("scratch_select", w_st["ms_select"])):
                        got[key].append(x)
            print(f"  {st['n_slabs']} slab(s); grown and from-scratch lists agree: {same}")
            for key, title in (("fill", "rows fill (device)"), ("select", "ms_select (device)"), ("finish", "finish (device)"), ("wall", "grown call wall"),
                               ("scratch", "from-scratch call wall"), ("scratch_select", "  its ms_select")):
                print(f"    {title:<24}{spread(got[key])}")
            print(f"    ratio scratch / grown   min {min(got['scratch']) / min(got['wall']):.1f}x   median "
                  f"{statistics.median(got['scratch']) / statistics.median(got['wall']):.1f}x")
        del square
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--phams", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slabs", type=int, default=0, help="also time the call cut into this many slabs (slab_bytes = dense bytes / this)")
    ap.add_argument("--configs", default=None, help="comma-separated metric:N:k triples instead of the default three")
    ap.add_argument("--rows", action="store_true", help="time the rows form (pc_fill_rows_nearest) against the fill from scratch instead")
    ap.add_argument("--new", default="5,50,500", help="with --rows: comma-separated counts of new genomes")
    a = ap.parse_args()
    if a.rows:
        return rows_mode(a)
    import numpy as np
    from phamclust_amd import hip
    from phamclust_amd.synth import synth_packed
    configs = [(c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in a.configs.split(",")] if a.configs else CONFIGS
    print(f"nearest-neighbours fill against dense fill + host selection: library version {hip.load().pc_version()}, {a.steps} calls after "
          f"{a.warmup} warm-up, ms")
    ctx, loaded = hip.Context(int(os.environ.get("PHAMCLUST_DEVICE", "0"))), None
    for metric, n, k in configs:
        pairs = n * (n - 1) // 2
        if loaded != (metric, n):
            ctx.upload(synth_packed(n, a.phams), residues=metric in hip.NEEDS_RESIDUES)
            loaded = (metric, n)
        print(f"\n{metric} synth({n},{a.phams}) k = {k}: {pairs:,} pairs, dense vector {pairs * 8 / 1e6:,.1f} MB, result {n * k * 12 / 1e6:,.2f} MB")
        for slab_bytes in (0,) + ((max(pairs * 8 // a.slabs, 8),) if a.slabs > 1 else ()):
            got = {key: [] for key in ("fill", "select", "finish", "wall", "dense", "dense_fill", "dense_select")}
            same = None
            for step in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                nbr, val, st = ctx.fill_nearest(metric, k, slab_bytes=slab_bytes, want_stats=True, borrow=True)
                wall = time.perf_counter() - t0
                nbr, val = np.array(nbr), np.array(val)
                d_nbr, d_val, fill_s, select_s = dense_route(ctx, metric, n, k)
                if same is None:
                    same = bool(np.array_equal(nbr, d_nbr) and np.array_equal(val, d_val))
                if step >= a.warmup:
                    for key, x in (("fill", st["ms_total"]), ("select", st["ms_select"]), ("finish", st["ms_finish"]), ("wall", wall * 1e3),
                                   ("dense", (fill_s + select_s) * 1e3), ("dense_fill", fill_s * 1e3), ("dense_select", select_s * 1e3)):
                        got[key].append(x)
            floor_bytes = 2 * 8 * pairs
            sel = min(got["select"])
            print(f"  slab_bytes {slab_bytes:,} ({st['n_slabs']} slab(s)); the two routes agree: {same}")
            for key, title in (("fill", "fill (device)"), ("select", "select (device)"), ("finish", "finish (device)"), ("wall", "call wall"),
                               ("dense", "dense route wall"), ("dense_fill", "  its fill + D2H"), ("dense_select", "  its host selection")):
                print(f"    {title:<22}{spread(got[key])}")
            print(f"    ratio dense / call    min {min(got['dense']) / min(got['wall']):.1f}x   median "
                  f"{statistics.median(got['dense']) / statistics.median(got['wall']):.1f}x")
            print(f"    selection floor       {floor_bytes / 1e9:.3f} GB (two reads of every slab) in {sel:.3f} ms = {floor_bytes / (sel * 1e-3) / 1e12:.2f} TB/s, "
                  f"{100.0 * floor_bytes / (sel * 1e-3) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak")
    ctx.close()


if __name__ == "__main__":
    main()
