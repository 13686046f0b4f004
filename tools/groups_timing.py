"""Time the groups fill (pc_fill_groups) where it is used: ``python tools/groups_timing.py`` writes ``profiles/groups_fill.txt``.

One process, one GPU.  Per workload -- ``synth_real(N)``, N = 5,000 and 20,000 by default, written as a TSV and read back through the
pipeline's loader -- and per metric (jc, peq), at the default ``clu`` distance (0.75):

* ``hierarchical_clustering_de_novo`` (one pack, one upload, one components fill, one groups fill) against the same function at the
  parent commit (a ``matrix_de_novo`` per component: a pack, an upload and a whole fill each).  The parent's ``clustering.py`` comes
  from ``--parent-clustering FILE``, else from ``git show 5159147:phamclust_amd/clustering.py`` (the commit is pinned).  Wall seconds, min / median of the
  steps after warm-up, and the share of them spent in pack + upload (the two are wrapped with a clock for the run).
* one groups fill over the components against the whole fill: HIP-event ms (pc_stats.ms_total) and wall seconds with the copy to
  the host, min / median.

The output file is written anew (``--append``: added to, each run under its own header line) and flushed line by line, so a run
that is cut short still leaves what it measured.
"""

import argparse
import importlib.util
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


PARENT_COMMIT = "5159147"          # the last commit whose hierarchical_clustering_de_novo fills component by component


def parent_module(path):
    """The parent route's module: ``path``, else ``phamclust_amd/clustering.py`` as of PARENT_COMMIT (pinned: HEAD^ is that commit
    only for the one commit that introduced the groups fill)."""
    text = open(path).read() if path else subprocess.run(["git", "-C", REPO, "show", f"{PARENT_COMMIT}:phamclust_amd/clustering.py"],
                                                         check=True, capture_output=True, text=True).stdout
    if "matrix_de_novo([by_name[name] for name in names]" not in text:
        raise SystemExit("groups_timing: the parent's clustering.py does not hold the per-component route (a matrix_de_novo per component)")
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "parent_clustering.py")
        with open(copy, "w") as handle:
            handle.write(text)
        spec = importlib.util.spec_from_file_location("parent_clustering", copy)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    return module


class Clock:
    """Accumulates the wall time of ``owner.name`` while installed."""

    def __init__(self, owner, name):
        self.owner, self.name, self.inner, self.seconds, self.calls = owner, name, getattr(owner, name), 0.0, 0

    def __enter__(self):
        def timed(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return self.inner(*args, **kwargs)
            finally:
                self.seconds += time.perf_counter() - t0
                self.calls += 1
        setattr(self.owner, self.name, timed)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self.inner)


def low_mid(values):
    return f"{min(values):9.3f} / {statistics.median(values):9.3f}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--genomes", type=int, nargs="+", default=[5000, 20000])
    ap.add_argument("--metrics", nargs="+", default=["jc", "peq"])
    ap.add_argument("--eps", type=float, default=0.75, help="distance threshold (default: the clu pass's, 1 - 0.25)")
    ap.add_argument("--linkage", default="average")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parent-clustering", default=None, help="the parent commit's phamclust_amd/clustering.py (default: git show 5159147:...)")
    ap.add_argument("--append", action="store_true", help="add to the output file instead of writing it anew")
    ap.add_argument("--skip-parent-above", type=int, default=0, help="skip the parent route for N above this (0: never)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "groups_fill.txt"))
    a = ap.parse_args()
    from phamclust_amd import cli, hip, matrix as M
    from phamclust_amd.clustering import hierarchical_clustering_de_novo
    from phamclust_amd.pack import load_tsv_genomes
    from phamclust_amd.synth import synth_real, write_tsv_packed
    parent = parent_module(a.parent_clustering)
    out = open(a.out, "a" if a.append else "w")
    scratch = tempfile.TemporaryDirectory()

    def say(line=""):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    try:
        import torch
        device = torch.cuda.get_device_name(int(os.environ.get("PHAMCLUST_DEVICE", "0")))
    except Exception:          # noqa: BLE001 -- the name is a label of the record, nothing more
        device = "unnamed device"
    say(f"groups fill on one {device}: library version {hip.load().pc_version()}, eps {a.eps}, linkage {a.linkage}, min / median of {a.steps} "
        f"after {a.warmup} warm-up; 'parent commit' = {PARENT_COMMIT} (a matrix_de_novo per component); clustering in wall seconds")
    for n in a.genomes:
        tsv = os.path.join(scratch.name, f"real_{n}.tsv")
        write_tsv_packed(synth_real(n), tsv)
        genomes = load_tsv_genomes(tsv)
        for metric in a.metrics:
            func = cli.METRICS[metric]
            ctx = M.get_context()
            t0 = time.perf_counter()
            packed = M._packed_of(genomes)
            t1 = time.perf_counter()
            ctx.upload(packed, residues=metric in ("aai", "peq"))
            t2 = time.perf_counter()
            labels = ctx.fill_components(metric, a.eps)
            groups = [g for g in M.Components(packed.names, labels).group_indices() if len(g) > 1]
            sizes = sorted((len(g) for g in groups), reverse=True)
            say(f"synth_real({n}) {metric}: {len(groups)} components of two or more (largest {sizes[:3]}), "
                f"{n - sum(sizes)} genomes alone; pack {t1 - t0:.3f} s, upload {t2 - t1:.3f} s")
            # one groups fill against the whole fill
            for label, call in (("groups fill", lambda: ctx.fill_groups(metric, groups, want_stats=True)),
                                ("whole fill ", lambda: ctx.fill(metric, want_stats=True, borrow=True))):
                ms, wall = [], []
                for k in range(a.warmup + a.steps):
                    t0 = time.perf_counter()
                    _, st = call()
                    if k >= a.warmup:
                        wall.append(time.perf_counter() - t0); ms.append(st["ms_total"])
                say(f"  {label}: {low_mid(ms)} ms on the device, {low_mid(wall)} s with the copy to the host; {st['n_pairs']:,} pairs, "
                    f"{st['n_alignments']:,} alignments, {st['n_distinct_alignments']:,} distinct, {st['n_chunks']} chunk(s)")
            # the clustering routes
            results = {}
            for label, route in (("this commit  ", hierarchical_clustering_de_novo), ("parent commit", parent.hierarchical_clustering_de_novo)):
                if route is parent.hierarchical_clustering_de_novo and a.skip_parent_above and n > a.skip_parent_above:
                    say(f"  {label}: skipped (N above --skip-parent-above)")
                    continue
                wall, share, calls = [], [], (0, 0)
                for k in range(a.warmup + a.steps):
                    with Clock(M, "_packed_of") as pack, Clock(hip.Context, "upload") as upload:
                        t0 = time.perf_counter()
                        parts = route(genomes, func, a.linkage, eps=a.eps)
                        seconds = time.perf_counter() - t0
                    if k >= a.warmup:
                        wall.append(seconds); share.append((pack.seconds + upload.seconds) / seconds); calls = (pack.calls, upload.calls)
                results[label] = ([p.nodes for p in parts], min(wall))
                say(f"  hierarchical_clustering_de_novo, {label}: {low_mid(wall)} s; pack + upload {100 * statistics.median(share):5.1f} % of it "
                    f"({calls[0]} packs, {calls[1]} uploads); {len(parts)} clusters")
            if len(results) == 2:
                (new_parts, new_s), (old_parts, old_s) = results.values()
                say(f"  same clusters: {new_parts == old_parts}; parent / this commit = {old_s / new_s:.2f} x (min over the steps)")
    out.close()
    scratch.cleanup()


if __name__ == "__main__":
    main()
