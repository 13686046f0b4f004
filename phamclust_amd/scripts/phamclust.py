"""The pipeline around the GPU matrix fill.

What it must stay compatible with is the reference's on-disk contract (scripts/phamclust.py:140-473), so that
caches and results interoperate: genomes sorted by name; cache directory ``<outdir>/<md5 of the FASTA text>.tmp``
holding ``01_genomes/<name>.fasta`` and ``02_distmats/<metric>_distance_matrix.tsv`` (lower triangle, reused when
present); three agglomerative passes (pre-group at ``nr``, cluster the group medoids at ``clu``, sub-cluster at
``sub``); ``cluster_<i>/`` (largest first) with ``genomes/*.faa``, ``<metric>_similarity.tsv``,
``subcluster_<j>_similarity.tsv`` and two heatmaps; ``singletons/genomes``; ``pairwise_<metric>_similarities.tsv`` and
``pairwise_<metric>_adjacency.tsv``.  Stage 2 is the only thing that changed: it is one GPU call.
"""

import hashlib
import logging
import pathlib
import shutil
import os
import sys
import time

import numpy as np

from phamclust_amd import distributed
from phamclust_amd import matrix as _matrix
from phamclust_amd import metrics as _metrics
from phamclust_amd.cli import METRICS, parse_args
from phamclust_amd.clustering import cluster_by_component, hierarchical_clustering
from phamclust_amd.genome import Genome
from phamclust_amd.heatmap import CSS_COLORS, draw_heatmap
from phamclust_amd.matrix import Components, GroupAffinity, GroupLinkage, PairDistribution, SparseEdges, SymMatrix, affinity_de_novo, between_de_novo, between_extend, between_from_file, between_to_file, components_de_novo, components_extend, components_from_file, components_to_file, distribution_de_novo, edges_de_novo, edges_to_adjacency, matrices_de_novo, matrix_de_novo, matrix_extend, matrix_from_squareform, matrix_to_adjacency, matrix_to_squareform, nearest_from_file, nearest_to_file, neighbors_de_novo, neighbors_extend, own_similarity_text, placement_de_novo, placement_report, stored_fit_from_file, tree_de_novo, tree_extend, tree_from_file, tree_to_file, upload_for_fills
from phamclust_amd.pack import load_tsv_genomes, packed_behind
from phamclust_amd import startup

LOG_STR_FMT = "phamclust: %(asctime)s.%(msecs)03d: %(levelname)s: %(message)s"
LOG_TIME_FMT = "%H:%M:%S"
FASTA_SUFFIXES = {".fasta", ".faa", ".fa"}
log = logging.getLogger()
TIMELINE = None                    # startup.Timeline of this run (main() makes it; library callers of phamclust() run without)
_PRELOADED = {}                    # infile -> genomes the CLI already loaded for its --gpus estimate


def _mark(name):
    if TIMELINE is not None:
        TIMELINE.mark(name)


def _gpus_text(st):
    """How many GPUs an edge-list, components or nearest fill ran on, for its log line: "1 GPU", or "N GPUs" with every device's
    stretch of targets and the times of the exchange and the merge."""
    n = st.get("n_gpus", 1)
    if n <= 1:
        return "1 GPU"
    bounds = st.get("stretches") or []
    parts = ", ".join(f"{a}..{b}" for a, b in zip(bounds, bounds[1:]))
    return f"{n} GPUs (targets {parts}; exchange {st.get('ms_exchange', 0.0):.3f} ms, merge {st.get('ms_merge', 0.0):.3f} ms)"


# ---- input ---------------------------------------------------------------------------------
def load_genomes_from_tsv(filepath):
    """Rows ``genome, pham[, translation]``; a missing translation is "M"; genomes in first-seen order."""
    found = {}
    with open(filepath) as handle:
        for number, line in enumerate(handle, start=1):
            fields = line.rstrip().split("\t")
            if len(fields) == 2:
                fields.append("M")
            if len(fields) != 3:
                raise ValueError("input file must either 2 or 3 columns")
            name, pham, translation = fields
            genome = found.get(name)
            if genome is None:
                genome = found[name] = Genome(name)
            genome.add(pham, translation)
    return list(found.values())


def load_genomes_from_fasta_dir(filepath):
    """One FASTA file per genome (stem = genome name; headers carry ``pham=``)."""
    found = {}
    for path in filepath.iterdir():
        if path.suffix not in FASTA_SUFFIXES or path.is_dir():
            log.debug(f"skipping {path}")
            continue
        if path.stem in found:
            raise ValueError(f"duplicate genome name detected {path.stem}")
        found[path.stem] = genome = Genome(path.stem)
        genome.load(path)
    return list(found.values())


def load_genomes(filepath):
    """TSV -> name-sorted genomes through the C loader (csrc/pc_pack.c): same genomes, same order, same FASTA text as
    ``sorted(load_genomes_from_tsv(filepath), key=name)`` (scripts/phamclust.py:21-47, 221), without a Python object
    per gene.  Translations with bytes outside ASCII take the Python loader."""
    try:
        return load_tsv_genomes(filepath)
    except ValueError as exc:
        if "non-ASCII" not in str(exc):
            raise
        return sorted(load_genomes_from_tsv(filepath), key=lambda g: g.name)


def read_pairs_file(filepath):
    """The pairs a ``--pairs`` file names: the first two tab-separated columns of every line, as (source name, target name) in file
    order.  Further columns are ignored, so an adjacency file of any metric is valid input; an empty line is skipped; a line with
    one column raises ``ValueError`` naming it."""
    pairs = []
    with open(filepath) as handle:
        for number, line in enumerate(handle, start=1):
            line = line.rstrip("\r\n")
            if not line:
                continue
            fields = line.split("\t")
            if len(fields) < 2 or not fields[0] or not fields[1]:
                raise ValueError(f"{filepath}, line {number}: expected two tab-separated genome names, got {line!r}")
            pairs.append((fields[0], fields[1]))
    return pairs


def _hash_genomes(genomes):
    """md5 of the concatenated FASTA text, genomes in the order given (the cache key)."""
    md5 = hashlib.md5()
    for genome in genomes:
        md5.update(genome.fasta_bytes() if hasattr(genome, "fasta_bytes") else str(genome).encode())
    return md5.hexdigest()


def check_matrix_integrity(matrix):
    """(edge-count error, diagonal-sum error, unfilled slots); all zero for a usable matrix.  The array-backed
    matrix cannot have the wrong number of edges, so the first term is always 0 here."""
    full = matrix.to_ndarray()
    upper = full[np.triu_indices(len(matrix))]
    return 0, float(np.nansum(full.diagonal())) - (0.0 if matrix.is_distance else float(len(matrix))), int(np.isnan(upper).sum())


# ---- the run -----------------------------------------------------------------------------------
class _Run:
    def __init__(self, outdir, metric, colors, midpoint):
        self.outdir, self.metric, self.colors, self.midpoint = outdir, metric, colors, midpoint
        self.genomes, self.by_name, self.cache, self.stage, self.fills = [], {}, None, None, None
        self.rank, self.world = 0, 1          # this process's place in the job (one process per GPU)
        self.extend = None                    # --extend FILE: a distance matrix over a subset of the genomes
        self.grow_nearest = None              # --grow-nearest FILE: a nearest_<metric>.tsv over a subset of the genomes
        self.grow = None                      # --grow FILE: a tree_<metric>.tsv / components_<metric>.tsv over a subset of the genomes
        self.also = []                        # --also: further metrics beside -m's, off the same joint fill
        self.also_matrices = {}               # ... their distance matrices, once stage 2 has run (distances_also)

    @staticmethod
    def _dir(path, fresh=False):
        if fresh and path.is_dir():
            shutil.rmtree(path)
        path.mkdir(exist_ok=True)
        return path

    def banner(self, number, title):
        now = time.perf_counter()
        if getattr(self, "_stage_t0", None) is not None:
            log.info(f"    ({now - self._stage_t0:.1f} s)")          # wall time of the stage that just ended
        self._stage_t0 = now
        log.info(f"--- {number}: {title} ---")

    # 1
    def read(self, infile, is_genome_dir):
        self.banner(1, "genomes")
        t0 = time.perf_counter()
        if is_genome_dir:
            self.genomes = sorted(load_genomes_from_fasta_dir(infile), key=lambda g: g.name)
        else:
            self.genomes = _PRELOADED.pop(str(infile), None) or load_genomes(infile)
        self.by_name = {g.name: g for g in self.genomes}
        log.info(f"loaded {len(self.genomes)} genomes in {time.perf_counter() - t0:.3f} s")
        _mark("load_genomes")
        if self.rank != 0:                    # the other ranks only need the genomes: rank 0 owns the output tree
            return
        digest = _hash_genomes(self.genomes)
        self.cache = self._dir(self.outdir / f"{digest}.tmp")
        log.info(f"{len(self.genomes)} genomes, md5 {digest}, cache {self.cache.name}")
        stash = self._dir(self.cache / "01_genomes")
        for genome in self.genomes:
            target = stash / f"{genome.name}.fasta"
            if not target.is_file():
                genome.save(target)

    # 2
    def distances(self, cpus):
        self.banner(2, f"{self.metric} distance matrix")
        cached, have_cache, failure = None, False, None
        if self.rank == 0:
            try:
                cached = self._dir(self.cache / "02_distmats") / f"{self.metric}_distance_matrix.tsv"
                have_cache = cached.is_file()
            except Exception as exc:          # noqa: BLE001 -- the other ranks must hear of it before they enter the gather
                if self.world == 1:
                    raise
                failure = exc
        if self.world > 1:                    # rank 0 owns the cache; the others learn whether there is work for them
            have_cache = distributed.broadcast_flag(have_cache, src=0, error=failure)
        t0 = time.perf_counter()
        if have_cache:
            if self.rank != 0:
                return None
            matrix = matrix_from_squareform(cached)
            log.info(f"read cached matrix in {time.perf_counter() - t0:.3f} s")
        elif self.extend is not None:
            matrix = self.extended(cpus, t0)
            matrix_to_squareform(matrix, cached, lower_triangle=True)
        else:
            matrix = matrix_de_novo(self.genomes, METRICS[self.metric], cpus)
            if matrix is None:                # not rank 0: this rank's shard went into the gather, nothing else to do
                return None
            wall = time.perf_counter() - t0
            st = _matrix.LAST_FILL
            pairs = st.get("genome_pairs", 0)
            line = (f"filled {len(matrix)} x {len(matrix)} matrix on {st.get('n_gpus', 1)} GPU(s) in {wall:.3f} s "
                    f"(pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, fill+gather+D2H {st.get('fill_s', 0.0):.3f}): "
                    f"{pairs / max(st.get('fill_s', 0.0), 1e-9):.3e} genome-pairs/s")
            if st.get("n_cells"):
                line += (f"; rank 0: {st['n_alignments']} alignments, {st['n_cells']:.3e} DP cells, "
                         f"{st['n_distinct_cells'] / max(st['ms_align'], 1e-6) / 1e6:.0f} GCUPS in the alignment kernels")
            log.info(line)
            peers = st.get("peer_access")                    # one process, N GPUs: how every shard reached the root -- never silent
            if peers:
                ways = ", ".join(f"{d['device']}: {d['access']}" for d in peers["devices"])
                log.info(f"exchange: device -> root copies {ways}; {st.get('ms_exchange', 0.0):.2f} ms (slowest copy)"
                         + (f"; STAGED THROUGH HOST for {peers['staged_through_host']} device(s): {peers['note']} "
                            f"(PHAMCLUST_MULTI=launcher gathers over RCCL instead)" if peers["staged_through_host"] else "")
                         + ("" if any(d["code"] == 1 for d in peers["devices"]) or peers["staged_through_host"] else
                            " [all contexts on the root's GPU: the cross-device branch did not run]"))
            if self.metric in _metrics.PARITY_NOTE:         # say it wherever these numbers leave the program
                log.info(f"parity: {_metrics.parity_note(self.metric)}")
            if TIMELINE is not None:                         # the matrix stage, split (matrix_de_novo's own clocks)
                TIMELINE.stamps += [("pack", st.get("pack_s", 0.0)), ("process_group_and_context", max(0.0, wall - st.get("pack_s", 0.0) - st.get("upload_s", 0.0) - st.get("fill_s", 0.0))),
                                    ("upload", st.get("upload_s", 0.0)), ("fill_exchange_d2h", st.get("fill_s", 0.0))]
                TIMELINE._last = time.time()
            matrix_to_squareform(matrix, cached, lower_triangle=True)
        if not matrix.is_distance:
            matrix.invert()
        edges, diagonal, unfilled = check_matrix_integrity(matrix)
        if edges or diagonal or unfilled:
            log.error(f"matrix failed integrity checks: edge count off by {edges}, diagonal off by {diagonal}, {unfilled} unfilled")
            print("matrix validation failed - check log for details")
            sys.exit(1)
        return matrix

    # 2, --also
    def distances_also(self, cpus):
        """Stage 2 with ``--also``: the distance matrices of -m's metric and of the ``--also`` metrics.  Those with a cache file under
        ``02_distmats/`` are read; the rest come from ONE ``matrices_de_novo`` call -- one pack, one upload, one joint fill when aai or peq
        is among them -- and each is cached as ``<metric>_distance_matrix.tsv``, the file a ``-m <metric>`` run caches.  Returns -m's matrix,
        on which the pipeline clusters exactly as without ``--also``; the others wait in ``also_matrices`` for ``finish``.  One process."""
        wanted = [self.metric] + self.also
        self.banner(2, f"{' + '.join(wanted)} distance matrices")
        folder = self._dir(self.cache / "02_distmats")
        found, missing = {}, []
        for name in wanted:
            cached = folder / f"{name}_distance_matrix.tsv"
            if cached.is_file():
                t0 = time.perf_counter()
                found[name] = matrix_from_squareform(cached)
                log.info(f"read cached {name} matrix in {time.perf_counter() - t0:.3f} s")
            else:
                missing.append(name)
        if missing:
            t0 = time.perf_counter()
            filled = matrices_de_novo(self.genomes, [METRICS[name] for name in missing], cpus)
            wall = time.perf_counter() - t0
            st = _matrix.LAST_FILL
            n = len(self.genomes)
            line = (f"filled {len(missing)} {n} x {n} matrices ({', '.join(missing)}) from {st.get('fills', 1)} fill(s) on 1 GPU in {wall:.3f} s "
                    f"(pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, fill+D2H {st.get('fill_s', 0.0):.3f}; kernels "
                    f"{st.get('ms_total', 0.0):.3f} ms, of which the walk that writes them {st.get('ms_reduce', 0.0):.3f} ms)")
            if st.get("n_cells"):
                line += (f": {st['n_alignments']} alignments ({st.get('n_distinct_alignments', 0)} distinct), {st['n_cells']:.3e} DP cells, "
                         f"{st.get('n_chunks', 1)} chunk(s), ONE alignment pass for all of them")
            log.info(line)
            noted = [name for name in missing if name in _metrics.PARITY_NOTE]
            if noted:                                       # say it wherever these numbers leave the program
                log.info(f"parity: {_metrics.parity_note(noted[0])}")
            for name in missing:
                matrix_to_squareform(filled[name], folder / f"{name}_distance_matrix.tsv", lower_triangle=True)
                found[name] = filled[name]
        for name in wanted:
            if not found[name].is_distance:
                found[name].invert()
            edges, diagonal, unfilled = check_matrix_integrity(found[name])
            if edges or diagonal or unfilled:
                log.error(f"{name} matrix failed integrity checks: edge count off by {edges}, diagonal off by {diagonal}, {unfilled} unfilled")
                print("matrix validation failed - check log for details")
                sys.exit(1)
        self.also_matrices = {name: found[name] for name in self.also}
        return found[self.metric]

    # 2, --adjacency-only
    def adjacency(self, similarity, prefilter=False):
        """Stage 2 as an edge-list fill: the pairs of similarity >= ``similarity`` (None: every non-zero one) straight into
        ``pairwise_<metric>_adjacency.tsv`` -- the file ``finish`` writes from the dense matrix (name order instead of cluster
        order), without the dense matrix: nothing is cached, nothing is clustered.  ``prefilter`` (peq, with a threshold): the same
        list behind its af bound (``edges_de_novo(..., prefilter=True)``)."""
        self.banner(2, f"{self.metric} adjacency (edge-list fill)")
        t0 = time.perf_counter()
        distance = 0.999999 if similarity is None else round(1.0 - similarity, 6)       # 6-place values: d <= 0.999999 is sim > 0
        edges = edges_de_novo(self.genomes, METRICS[self.metric], distance, as_distance=True, prefilter=prefilter)
        st = _matrix.LAST_FILL
        pairs = st.get("genome_pairs", 0)
        if prefilter:
            log.info(f"--prefilter: {st.get('n_candidates', 0):,} of {pairs:,} pairs are af candidates; {st.get('n_alignments', 0):,} alignments "
                     f"({st.get('n_distinct_alignments', 0):,} distinct) behind them")
        log.info(f"{len(edges):,} of {pairs:,} pairs ({100.0 * len(edges) / max(pairs, 1):.1f} %) within distance {distance:.6f} from "
                 f"{st.get('n_slabs', 1)} slab(s) on {_gpus_text(st)} in {time.perf_counter() - t0:.3f} s (pack {st.get('pack_s', 0.0):.3f}, upload "
                 f"{st.get('upload_s', 0.0):.3f}, fill+compact+D2H {st.get('fill_s', 0.0):.3f}; kernels {st.get('ms_total', 0.0):.3f} ms, "
                 f"compaction {st.get('ms_compact', 0.0):.3f} ms, edge copy {st.get('ms_d2h', 0.0):.3f} ms)")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        target = self.outdir / f"pairwise_{self.metric}_adjacency.tsv"
        edges_to_adjacency(edges.inverted(), target, skip_zero=True)
        log.info(f"wrote {target.name}")
        return edges

    # 2, --pairs
    def pairs(self, listing):
        """Stage 2 as a pair-list fill: the pairs ``listing`` names (``read_pairs_file``), each oriented as written, into
        ``pairwise_<metric>_pairs.tsv`` as ``source<TAB>target<TAB>similarity`` in the listing's order.  Nothing else is computed.  With
        ``--also``: ONE joint pair-list fill for -m's metric and the ``--also`` metrics, and one such file per metric."""
        wanted = [self.metric] + self.also
        self.banner(2, f"{' + '.join(wanted)} of the listed pairs (pair-list fill)")
        t0 = time.perf_counter()
        named = read_pairs_file(listing)
        if self.also:
            values = _matrix.pairs_joint_de_novo(self.genomes, [METRICS[name] for name in wanted], named, as_distance=False)
        else:
            values = {self.metric: _matrix.pairs_de_novo(self.genomes, METRICS[self.metric], named, as_distance=False)}
        st = _matrix.LAST_FILL
        log.info(f"{len(named):,} listed pairs ({st.get('n_pairs', 0):,} off the diagonal) of {len(self.genomes):,} genomes on 1 GPU in "
                 f"{time.perf_counter() - t0:.3f} s (pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, sort+fill+D2H "
                 f"{st.get('fill_s', 0.0):.3f}; kernels {st.get('ms_total', 0.0):.3f} ms)"
                 + (f"; {len(wanted)} metrics from {st.get('fills', 1)} fill(s): {st.get('n_alignments', 0):,} alignments "
                    f"({st.get('n_distinct_alignments', 0):,} distinct) in {st.get('n_chunks', 1)} chunk(s), ONE alignment pass for all of them"
                    if self.also else ""))
        noted = [name for name in wanted if name in _metrics.PARITY_NOTE]
        if noted:
            log.info(f"parity: {_metrics.parity_note(noted[0])}")
        for name in wanted:
            target = self.outdir / f"pairwise_{name}_pairs.tsv"
            with open(target, "w") as handle:
                for (source, other), value in zip(named, values[name].tolist()):
                    handle.write(f"{source}\t{other}\t{value:.6f}\n")
            log.info(f"wrote {target.name}")
        return values[self.metric]

    # 2, --components-only
    def components(self, similarity):
        """Stage 2 as a components fill: genomes are joined when their distance is below ``round(1 - similarity, 6)`` -- the
        single-linkage groups at that eps -- and only ``components_<metric>.tsv`` is written: ``name<TAB>number`` in genome order,
        number 1 for the largest group (``Components.groups()``'s order).  No matrix, no edge list, nothing cached or clustered."""
        self.banner(2, f"{self.metric} components (components fill)")
        t0 = time.perf_counter()
        distance = round(1.0 - similarity, 6)
        if self.grow is not None:
            found = self.grown(lambda: components_from_file(self.grow),
                               lambda old: components_extend(old, self.genomes, METRICS[self.metric], distance, strict=True, as_distance=True), t0)
        else:
            found = components_de_novo(self.genomes, METRICS[self.metric], distance, as_distance=True, strict=True)
        st = _matrix.LAST_FILL
        groups = found.group_indices()
        log.info(f"{len(self.genomes):,} genomes, {st.get('n_edges', 0):,} of {st.get('genome_pairs', 0):,} pairs within distance < {distance:.6f}: "
                 f"{len(groups):,} components, the largest of {len(groups[0]) if groups else 0:,}, from {st.get('n_slabs', 1)} slab(s) on {_gpus_text(st)} in "
                 f"{time.perf_counter() - t0:.3f} s (pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, fill+union+labels "
                 f"{st.get('fill_s', 0.0):.3f}; kernels {st.get('ms_total', 0.0):.3f} ms, union {st.get('ms_union', 0.0):.3f} ms, labels "
                 f"{st.get('ms_labels', 0.0):.3f} ms)")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        target = self.outdir / f"components_{self.metric}.tsv"
        components_to_file(found, target)
        log.info(f"wrote {target.name}")
        return found

    # 2, --nearest
    def nearest(self, k, bound=False):
        """Stage 2 as a nearest-neighbours fill: each genome's ``k`` closest genomes, and only ``nearest_<metric>.tsv`` is written:
        ``source<TAB>target<TAB>similarity``, sources in genome order, targets nearest first (equally near ones in genome order).
        Distances are filled and inverted, as for the adjacency file.  No matrix, no threshold, nothing cached or clustered.
        ``bound`` (peq): the same lists behind the af bound (``neighbors_de_novo(..., bound=True)``)."""
        self.banner(2, f"{self.metric} nearest neighbours (nearest-neighbours fill)")
        t0 = time.perf_counter()
        if self.grow_nearest is not None:
            names = [g.name for g in self.genomes]
            found = self.grown(lambda: nearest_from_file(self.grow_nearest, names),
                               lambda old: neighbors_extend(old, self.genomes, METRICS[self.metric], k=k), t0, flag="--grow-nearest", path=self.grow_nearest)
        else:
            found = neighbors_de_novo(self.genomes, METRICS[self.metric], k, as_distance=True, bound=bound)
        st = _matrix.LAST_FILL
        if bound:
            pairs = st.get("genome_pairs", 0)
            log.info(f"--af-bound: {st.get('n_candidates', 0):,} of {pairs:,} pairs are af candidates ({st.get('n_seed_pairs', 0):,} seed pairs)"
                     f"{'; more than half: fell back to the plain fill' if st.get('fallback') else ''}; {st.get('n_alignments', 0):,} alignments against "
                     f"{pairs:,} pairs x the mean a plain fill aligns")
        log.info(f"{st.get('genome_pairs', 0):,} pairs -> the {found.k} nearest of each of {len(found):,} genomes from {st.get('n_slabs', 1)} slab(s) "
                 f"on {_gpus_text(st)} in {time.perf_counter() - t0:.3f} s (pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, "
                 f"fill+select+D2H {st.get('fill_s', 0.0):.3f}; kernels {st.get('ms_total', 0.0):.3f} ms, selection "
                 f"{st.get('ms_select', 0.0):.3f} ms, finish {st.get('ms_finish', 0.0):.3f} ms)")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        target = self.outdir / f"nearest_{self.metric}.tsv"
        nearest_to_file(found, target)
        log.info(f"wrote {target.name}")
        return found

    # 2, --place
    def place(self, path, verify=4):
        """Stage 2 as a placement: ``path`` is the ``cluster_fit_<metric>.tsv`` of an earlier run over a subset of the genomes; the genomes
        it lacks are placed against its clusters by ONE rows form of the affinity fill, and only ``placement_<metric>.tsv`` is written
        (``placement_report``).  The new genomes stay in no cluster, so the own entry of an old genome is over old members only:
        ``verify`` old genomes ride along as queries and their own-similarity text must be the file's, byte for byte -- the guard against
        a stale file, another metric or changed genomes."""
        self.banner(2, f"{self.metric} placement of new genomes (rows form of the affinity fill)")
        t0 = time.perf_counter()
        names = [g.name for g in self.genomes]
        try:
            clusters, groups, own = stored_fit_from_file(path)
            there = set(names)
            missing = next((name for group in groups for name in group if name not in there), None)
            if missing is not None:
                raise KeyError(f"genome '{missing}' of the file is not among the genomes of the input")
            if len(groups) > _matrix.BETWEEN_MAX_GROUPS:
                raise ValueError(f"{len(groups):,} clusters are above the fill's {_matrix.BETWEEN_MAX_GROUPS:,} groups")
            new = [name for name in names if name not in own]
            old = [name for name in names if name in own]
            several = {name for group in groups if len(group) > 1 for name in group}        # (a genome alone in its cluster has no own similarity to hold)
            pool = [name for name in old if name in several] or old
            n_verify = max(0, min(int(verify), len(pool)))
            checked = sorted({pool[(i * len(pool)) // n_verify] for i in range(n_verify)}, key=names.index)
            found = placement_de_novo(self.genomes, METRICS[self.metric], groups, queries=new + checked, as_distance=True)
            for name in checked:
                if own_similarity_text(found, name) != own[name]:
                    raise ValueError(f"genome '{name}': the file holds the own similarity {own[name]}, the {self.metric} fill gives "
                                     f"{own_similarity_text(found, name)}: the file was not written with this metric from these genomes")
        except (ValueError, KeyError, OSError) as exc:
            log.error(f"--place {path}: {exc.args[0] if isinstance(exc, KeyError) and exc.args else exc}")
            print("placing the new genomes failed - check log for details")
            sys.exit(1)
        st = _matrix.LAST_FILL
        log.info(f"placed {len(new):,} new genomes against {len(groups):,} clusters of {len(old):,} genomes ({len(checked)} of them verified): "
                 f"{st.get('genome_pairs', 0):,} pairs filled instead of {len(names) * (len(names) - 1) // 2:,} in {time.perf_counter() - t0:.3f} s "
                 f"(pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, fill+passes+D2H {st.get('fill_s', 0.0):.3f}; kernels "
                 f"{st.get('ms_total', 0.0):.3f} ms, row passes {st.get('ms_rows', 0.0):.3f} ms, finish {st.get('ms_finish', 0.0):.3f} ms)")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        target = self.outdir / f"placement_{self.metric}.tsv"
        with open(target, "w") as handle:
            handle.write("\n".join(placement_report(found, clusters, new)) + "\n")
        log.info(f"wrote {target.name}")
        return found

    # 2, --place --grow-table
    def grow_table(self, fit_path, table_path, found, join_min=None):
        """After ``place``: the stored ``cluster_table_<metric>.tsv`` at ``table_path`` -- of the run that wrote ``fit_path`` -- grown by the
        new genomes.  Every new genome joins its ``assigned("mean")`` cluster of ``found``; with ``join_min`` a genome whose nearest mean
        similarity lies below it (and one no cluster is near) becomes a singleton group, appended after the stored groups in genome order
        and named by the genome.  ``between_extend`` fills only the new genomes' pairs and verifies whole old clusters against the file;
        writes ``cluster_table_<metric>.tsv`` into the output directory.  A failure is logged and exits 1 without writing the table."""
        self.banner("2b", f"{self.metric} cluster table grown by the placed genomes (rows form of the between-groups fill)")
        t0 = time.perf_counter()
        names = [g.name for g in self.genomes]
        try:
            clusters, fit_groups, own = stored_fit_from_file(fit_path)
            at = {cluster: k for k, cluster in enumerate(clusters)}
            table_names, _ = between_from_file(table_path, None, is_distance=False)
            stranger = next((name for name in table_names if name not in at), None)
            if stranger is not None:
                raise ValueError(f"group '{stranger}' of the table is no cluster of {fit_path}")
            if len(table_names) != len(clusters):
                raise ValueError(f"the table holds {len(table_names)} groups, {fit_path} {len(clusters)} clusters")
            table_names, stored = between_from_file(table_path, [fit_groups[at[name]] for name in table_names], is_distance=False)
            new = [name for name in names if name not in own]
            joined = found.assigned("mean", min_similarity=join_min)
            groups = [list(group) for group in stored.groups]
            singles = []
            for name in new:
                k = joined.get(name)
                if k is None:
                    singles.append(name)
                else:
                    groups[table_names.index(clusters[k])].append(name)
            taken = next((name for name in singles if name in at), None)
            if taken is not None:
                raise ValueError(f"new genome '{taken}' would name a singleton group, and the table has a group of that name")
            table = between_extend(stored, self.genomes, METRICS[self.metric], groups + [[name] for name in singles])
        except (ValueError, KeyError, OSError, RuntimeError) as exc:
            log.error(f"--grow-table {table_path}: {exc.args[0] if isinstance(exc, KeyError) and exc.args else exc}")
            print("growing the cluster table failed - check log for details")
            sys.exit(1)
        st = _matrix.LAST_FILL
        log.info(f"grew the table of {len(stored):,} clusters by {len(new):,} genomes ({len(new) - len(singles):,} joined a cluster, {len(singles):,} "
                 f"became singletons; {st.get('verified_rows', 0)} old genomes verified): {int(st.get('n_pairs', 0)):,} pairs filled instead of "
                 f"{len(names) * (len(names) - 1) // 2:,} in {time.perf_counter() - t0:.3f} s (kernels {st.get('ms_total', 0.0):.3f} ms, pass "
                 f"{st.get('ms_reduce', 0.0):.3f} ms, fold {st.get('ms_finish', 0.0):.3f} ms)")
        target = self.outdir / f"cluster_table_{self.metric}.tsv"
        between_to_file(table, table_names + singles, target)
        log.info(f"wrote {target.name}")
        return table

    # 2, --tree
    def tree(self):
        """Stage 2 as a tree fill: the single-linkage dendrogram, and only ``tree_<metric>.tsv`` is written: one
        ``source<TAB>target<TAB>similarity`` line per edge of the minimum spanning tree, in merge order (the most similar pair first;
        equal similarities by target, then source, in genome order).  Distances are filled and inverted, as for the adjacency file.
        No matrix, no threshold, nothing cached or clustered."""
        self.banner(2, f"{self.metric} single-linkage tree (tree fill)")
        t0 = time.perf_counter()
        if self.grow is not None:
            names = [g.name for g in self.genomes]
            found = self.grown(lambda: tree_from_file(self.grow, names), lambda old: tree_extend(old, self.genomes, METRICS[self.metric]), t0)
        else:
            found = tree_de_novo(self.genomes, METRICS[self.metric], as_distance=True)
        st = _matrix.LAST_FILL
        log.info(f"{st.get('genome_pairs', 0):,} pairs -> the {len(found):,} edges of the single-linkage tree of {len(found.nodes):,} genomes from "
                 f"{st.get('n_slabs', 1)} slab(s) on {_gpus_text(st)} in {time.perf_counter() - t0:.3f} s (pack {st.get('pack_s', 0.0):.3f}, upload "
                 f"{st.get('upload_s', 0.0):.3f}, fill+rounds+D2H {st.get('fill_s', 0.0):.3f}; kernels {st.get('ms_total', 0.0):.3f} ms, rounds "
                 f"{st.get('ms_rounds', 0.0):.3f} ms, finish {st.get('ms_finish', 0.0):.3f} ms)")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        target = self.outdir / f"tree_{self.metric}.tsv"
        tree_to_file(found, target)
        log.info(f"wrote {target.name}")
        return found

    def grown(self, read, extend, t0, flag="--grow", path=None):
        """Stage 2 under --grow / --grow-nearest: the stored tree, components or nearest-neighbour lists are read back, held against a
        refill of a few old genomes and grown by the rows of the genomes they lack (tree_extend / components_extend / neighbors_extend)."""
        try:
            old = read()
            found = extend(old)
        except (ValueError, KeyError, OSError) as exc:
            log.error(f"{flag} {self.grow if path is None else path}: {exc.args[0] if isinstance(exc, KeyError) and exc.args else exc}")
            print("growing the stored result failed - check log for details")
            sys.exit(1)
        st, n = _matrix.LAST_FILL, len(found.nodes)
        added = n - len(old.nodes)
        rows, filled = (st.get("rows", added), st.get("genome_pairs", 0)) if added else (0, 0)      # (nothing new: no fill ran)
        log.info(f"grown {len(old.nodes):,} -> {n:,} genomes: {rows:,} rows, {filled:,} pairs filled instead of {n * (n - 1) // 2:,} in "
                 f"{time.perf_counter() - t0:.3f} s")
        if not added:
            _matrix.LAST_FILL.clear()
        return found

    def extended(self, cpus, t0):
        """Stage 2 under --extend: the old matrix's block is kept, the rows of the genomes it lacks are filled (matrix_extend)."""
        try:
            old = matrix_from_squareform(self.extend)
            if not old.is_distance:
                raise ValueError(f"'{self.extend}' holds similarities; --extend takes the distance matrix a run wrote (02_distmats/)")
            matrix = matrix_extend(old, self.genomes, METRICS[self.metric], cpus)
        except (ValueError, KeyError, OSError) as exc:
            log.error(f"--extend {self.extend}: {exc.args[0] if isinstance(exc, KeyError) and exc.args else exc}")
            print("matrix extension failed - check log for details")
            sys.exit(1)
        st, n = _matrix.LAST_FILL, len(matrix)
        added = n - len(old)
        filled = st.get("genome_pairs", added * (n - 1) - added * (added - 1) // 2) if added else 0
        log.info(f"extended {len(old):,} -> {n:,} genomes: {st.get('rows', added) if added else 0:,} rows, {filled:,} pairs filled instead of "
                 f"{n * (n - 1) // 2:,} in {time.perf_counter() - t0:.3f} s")
        if added and self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        return matrix

    # 3
    def clusters(self, matrix, nr, clu):
        self.banner(3, "clusters")
        groups = hierarchical_clustering(matrix, eps=nr[0], linkage=nr[1])          # near-identical genomes
        by_medoid = {group.medoid[0]: group for group in groups}
        medoids = matrix.extract_submatrix(list(by_medoid))
        merged = []
        for cluster in hierarchical_clustering(medoids, eps=clu[0], linkage=clu[1]):
            members = [node for medoid in cluster.nodes for node in by_medoid[medoid].nodes]
            merged.append(matrix.extract_submatrix(members))
        multi = sorted((m for m in merged if len(m) > 1), reverse=True)
        single = [m for m in merged if len(m) == 1]
        log.info(f"{len(groups)} pre-groups -> {len(multi)} clusters + {len(single)} singletons")
        return multi, single

    # 2 + 3, --no-matrix
    def clusters_no_matrix(self, nr, clu):
        """Stages 2 and 3 without the dense matrix: what ``clusters(distances(), nr, clu)`` returns, from ONE upload, two components
        fills (N labels each) and three groups fills (the sub-matrices, sum of n_c^2 cells).  Every pass clusters component by
        component (``cluster_by_component``: a cluster cut at eps never spans two components of {d < eps}), so its parts and their
        order are the dense route's."""
        self.banner(2, f"{self.metric} clusters without the dense matrix (components and groups fills)")
        t0 = time.perf_counter()
        ctx, metric, names, _ = upload_for_fills(self.genomes, METRICS[self.metric], "--no-matrix")
        self.fills = (ctx, metric, names)                   # finish_no_matrix fills the adjacency file's edges on the same upload
        index = {name: k for k, name in enumerate(names)}
        filled = [0, 0]

        def submatrices(groups):
            """One groups fill: the distance matrix of each group of names, its nodes in the group's own order."""
            out = [None] * len(groups)
            multi = [k for k, group in enumerate(groups) if len(group) > 1]
            ascending = [sorted(index[name] for name in groups[k]) for k in multi]
            values, st = ctx.fill_groups(metric, ascending, as_distance=True, want_stats=True)
            filled[0] += 1; filled[1] += int(st["n_pairs"])
            for k, idx, condensed in zip(multi, ascending, values):
                block = SymMatrix.from_condensed([names[i] for i in idx], condensed, is_distance=True)
                out[k] = block if block.nodes == list(groups[k]) else block.extract_submatrix(list(groups[k]))
            for k, group in enumerate(groups):
                if out[k] is None:
                    out[k] = SymMatrix(nodes=list(group), is_distance=True)
                    for node in group:
                        out[k].set_weight(node, node, 0.0)
            return out

        # near-identical genomes: the components at nr, each clustered alone with the nr linkage
        near = Components(names, ctx.fill_components(metric, nr[0], as_distance=True, strict=True)).groups()
        of_first = {m.nodes[0]: m for m in submatrices([g for g in near if len(g) > 1])}
        groups = cluster_by_component(near, lambda group: of_first[group[0]], nr[1], nr[0], nodes=names)
        by_medoid = {group.medoid[0]: group for group in groups}
        # the medoids: the components at clu over ALL genomes are no finer than the medoids' own, so no cluster of medoids spans two
        order = {medoid: k for k, medoid in enumerate(by_medoid)}
        wide = Components(names, ctx.fill_components(metric, clu[0], as_distance=True, strict=True)).groups()
        medoid_groups = [sorted((name for name in group if name in order), key=order.__getitem__) for group in wide]
        medoid_groups = [group for group in medoid_groups if group]
        of_first = {m.nodes[0]: m for m in submatrices(medoid_groups)}
        merged = []
        for cluster in cluster_by_component(medoid_groups, lambda group: of_first[group[0]], clu[1], clu[0], nodes=list(by_medoid)):
            merged.append([node for medoid in cluster.nodes for node in by_medoid[medoid].nodes])
        merged = submatrices(merged)
        multi = sorted((m for m in merged if len(m) > 1), reverse=True)
        single = [m for m in merged if len(m) == 1]
        n = len(names)
        log.info(f"{len(groups)} pre-groups -> {len(multi)} clusters + {len(single)} singletons in {time.perf_counter() - t0:.3f} s: one upload, "
                 f"2 components fills, {filled[0]} groups fills of {filled[1]:,} pairs in all instead of {n * (n - 1) // 2:,}")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        return multi, single

    # 4
    def write_cluster(self, number, cluster, sub, k_min, no_sub):
        root = self._dir(self.stage / f"cluster_{number}", fresh=True)
        faa = self._dir(root / "genomes")
        members = set(cluster.nodes)
        for genome in self.genomes:
            if genome.name in members:
                genome.save(faa / f"{genome.name}.faa")
        if no_sub or len(cluster) < k_min:
            cluster.reorder()
        else:
            order = []
            parts = sorted(hierarchical_clustering(cluster, eps=sub[0], linkage=sub[1]), reverse=True)
            for j, part in enumerate(parts, start=1):
                if len(part) > 2:
                    part.reorder()
                order += part.nodes
                matrix_to_squareform(part.invert(), root / f"subcluster_{j}_similarity.tsv")
            cluster.reorder(order)
        matrix_to_squareform(cluster.invert(), root / f"{self.metric}_similarity.tsv")
        for suffix in ("svg", "html"):
            draw_heatmap(cluster, colors=self.colors, midpoint=self.midpoint, filename=root / f"{self.metric}_heatmap.{suffix}")

    # 4b, --cluster-table
    def cluster_table(self, groups, clu_distance):
        """One between-groups fill over the final clusters -- ``groups``: the multi-genome clusters in output order, then the singletons,
        as lists of names -- into the staging directory: ``cluster_table_<metric>.tsv`` (the long form, similarities),
        ``cluster_<metric>_similarities.tsv`` (the mean similarity of every two clusters as a square over ``cluster_1 .. cluster_k`` and
        the singletons' names; the diagonal a cluster's own mean) and, for at most 1,500 clusters, the heatmap of that square.  On the
        --no-matrix route the fill runs on the upload that route holds; else on one of its own, over the devices of this process."""
        self.banner("4b", f"{self.metric} cluster table (between-groups fill)")
        t0 = time.perf_counter()
        if len(groups) > _matrix.BETWEEN_MAX_GROUPS:
            log.warning(f"--cluster-table: {len(groups):,} clusters and singletons are above the fill's {_matrix.BETWEEN_MAX_GROUPS:,} groups: "
                        f"no cluster table is written")
            return None
        multi = sum(1 for group in groups if len(group) > 1)
        names = [f"cluster_{k + 1}" if k < multi else group[0] for k, group in enumerate(groups)]
        if self.fills is not None:
            ctx, metric, genome_names = self.fills
            index = {name: k for k, name in enumerate(genome_names)}
            label = np.zeros(len(genome_names), dtype=np.int32)
            for k, group in enumerate(groups):
                label[[index[name] for name in group]] = k
            *arrays, st = ctx.fill_between(metric, label, len(groups), as_distance=True, want_stats=True)
            table = GroupLinkage(groups, *arrays, is_distance=True)
        else:
            table = between_de_novo(self.genomes, METRICS[self.metric], groups, as_distance=True)
            st = _matrix.LAST_FILL
        log.info(f"{len(groups):,} clusters and singletons -> {len(groups) * (len(groups) + 1) // 2:,} entries from {st.get('n_slabs', 1)} slab(s) on "
                 f"{_gpus_text(st)} in {time.perf_counter() - t0:.3f} s (kernels {st.get('ms_total', 0.0):.3f} ms, reduction "
                 f"{st.get('ms_reduce', 0.0):.3f} ms, finish {st.get('ms_finish', 0.0):.3f} ms)")
        table = table.inverted()
        between_to_file(table, names, self.stage / f"cluster_table_{self.metric}.tsv")
        square = table.to_symmatrix(names, "mean")
        matrix_to_squareform(square, self.stage / f"cluster_{self.metric}_similarities.tsv")
        if len(groups) > 1500:
            log.info("cluster table too large for a heatmap")
        else:
            for suffix in ("html", "svg"):
                draw_heatmap(square, colors=self.colors, midpoint=1.0 - clu_distance, filename=self.stage / f"cluster_{self.metric}_heatmap.{suffix}")
        return table

    # 4c, --cluster-fit
    def cluster_fit(self, groups):
        """One affinity fill over the final clusters (``groups`` as ``cluster_table`` takes them) into the staging directory:
        ``cluster_fit_<metric>.tsv``, one line per genome in cluster order -- its cluster, its mean similarity to its own cluster, the
        nearest other cluster by mean and that mean, its silhouette, whether it is its cluster's medoid -- and
        ``cluster_fit_<metric>_summary.tsv``, one line per cluster: size, medoid, mean silhouette, largest own distance.  The fill runs
        where ``cluster_table``'s does; the numbers are exact integers on every route, so the files are the same on all of them."""
        self.banner("4c", f"{self.metric} cluster fit (affinity fill)")
        t0 = time.perf_counter()
        if len(groups) > _matrix.BETWEEN_MAX_GROUPS:
            log.warning(f"--cluster-fit: {len(groups):,} clusters and singletons are above the fill's {_matrix.BETWEEN_MAX_GROUPS:,} groups: "
                        f"no cluster fit is written")
            return None
        multi = sum(1 for group in groups if len(group) > 1)
        names = [f"cluster_{k + 1}" if k < multi else group[0] for k, group in enumerate(groups)]
        if self.fills is not None:
            ctx, metric, genome_names = self.fills
            index = {name: k for k, name in enumerate(genome_names)}
            label = np.zeros(len(genome_names), dtype=np.int32)
            for k, group in enumerate(groups):
                label[[index[name] for name in group]] = k
            found = ctx.fill_affinity(metric, label, len(groups), as_distance=True, want_stats=True)
            st = found.pop("stats")
            found.pop("table")
            fit = GroupAffinity(genome_names, groups, **found, is_distance=True)
        else:
            fit = affinity_de_novo(self.genomes, METRICS[self.metric], groups, as_distance=True)
            st = _matrix.LAST_FILL
        log.info(f"{len(fit):,} genomes x {len(groups):,} clusters and singletons from {st.get('n_slabs', 1)} slab(s) on {_gpus_text(st)} in "
                 f"{time.perf_counter() - t0:.3f} s (kernels {st.get('ms_total', 0.0):.3f} ms, row passes {st.get('ms_rows', 0.0):.3f} ms, column passes "
                 f"{st.get('ms_cols', 0.0):.3f} ms, finish {st.get('ms_finish', 0.0):.3f} ms)")
        at = {name: k for k, name in enumerate(fit.nodes)}
        silhouette, medoids, by_group = fit.silhouette(), fit.medoids(), fit.silhouette_by_group()
        similar = fit.inverted()                                            # (similarities from the integers, as every output of the run)
        near, near_mean = fit.nearest_group("mean"), similar.nearest_value("mean")

        def text(value):
            return "nan" if value != value else repr(float(value))

        with open(self.stage / f"cluster_fit_{self.metric}.tsv", "w") as handle:
            handle.write("genome\tcluster\town_similarity\tnearest_cluster\tnearest_similarity\tsilhouette\tmedoid\n")
            for b, group in enumerate(groups):
                for name in group:
                    k = at[name]
                    handle.write(f"{name}\t{names[b]}\t{text(similar.own_mean(name))}\t{names[near[k]] if near[k] >= 0 else 'none'}\t{text(near_mean[k])}\t"
                                 f"{text(silhouette[k])}\t{int(medoids[b] == name)}\n")
        with open(self.stage / f"cluster_fit_{self.metric}_summary.tsv", "w") as handle:
            handle.write("cluster\tsize\tmedoid\tmean_silhouette\tlargest_own_distance\n")
            for b, group in enumerate(groups):
                worst = max(int(fit.own_hi[at[name]]) for name in group)
                handle.write(f"{names[b]}\t{len(group)}\t{medoids[b]}\t{text(by_group[b])}\t{'nan' if worst < 0 else f'{worst / 1.0e6:.6f}'}\n")
        log.info(f"mean silhouette of the {len(groups):,} clusters and singletons: {text(fit.silhouette_mean())}")
        return fit

    def _distribution_files(self, found, folder, thresholds, clu_similarity=None):
        """The two files of a distribution -- ``found``, similarities -- into ``folder``: the non-empty bins, and the summary, one
        ``statistic<TAB>value`` line each: n, min, max, mean, std, skew (``SymMatrix.statistics``' forms, from exact integers), the
        quartiles, the pairs that pass each of ``thresholds`` (name, similarity) and, for a split distribution, how ``clu_similarity``
        separates the clusters and the threshold that would separate them best."""
        found.to_file(folder / f"pairwise_{self.metric}_distribution.tsv")
        rows = [("n", f"{found.n_pairs}")]
        if found.n_pairs:
            mean, std, skew = found.statistics
            rows += [("min", f"{found.min:.6f}"), ("max", f"{found.max:.6f}"), ("mean", repr(mean)), ("std", repr(std)), ("skew", repr(skew)),
                     ("q25", f"{found.quantile(0.25):.6f}"), ("median", f"{found.median:.6f}"), ("q75", f"{found.quantile(0.75):.6f}")]
        rows += [(f"pairs_at_{name}_{value:.6f}", f"{found.count_within(value)}") for name, value in thresholds]
        if found.partitioned:
            rows += [("within_pairs", f"{found.within.n_pairs}"), ("between_pairs", f"{found.between.n_pairs}")]
            beyond, inside = found.separation(clu_similarity)
            rows += [(f"within_beyond_clu_thresh_{clu_similarity:.6f}", f"{beyond}"), (f"between_inside_clu_thresh_{clu_similarity:.6f}", f"{inside}")]
            best, beyond, inside = found.best_separation()
            rows += [("best_separation", f"{best:.6f}"), ("best_separation_within_beyond", f"{beyond}"), ("best_separation_between_inside", f"{inside}")]
        with open(folder / f"pairwise_{self.metric}_distribution_summary.tsv", "w") as handle:
            handle.writelines(f"{key}\t{value}\n" for key, value in rows)
        log.info(f"wrote pairwise_{self.metric}_distribution.tsv ({found.micro.shape[0]:,} occupied bins) and pairwise_{self.metric}_distribution_summary.tsv")

    # 2, --distribution-only
    def distribution(self, thresholds):
        """Stage 2 as a distribution fill: the exact histogram of all pair values, and only its two files are written.  Distances are
        filled and inverted, as for the adjacency file.  No matrix, no threshold, nothing cached or clustered."""
        self.banner(2, f"{self.metric} pair distribution (distribution fill)")
        t0 = time.perf_counter()
        found = distribution_de_novo(self.genomes, METRICS[self.metric], as_distance=True)
        st = _matrix.LAST_FILL
        log.info(f"{st.get('genome_pairs', 0):,} pairs -> {found.micro.shape[0]:,} occupied bins from {st.get('n_slabs', 1)} slab(s) on {_gpus_text(st)} in "
                 f"{time.perf_counter() - t0:.3f} s (pack {st.get('pack_s', 0.0):.3f}, upload {st.get('upload_s', 0.0):.3f}, fill+count+D2H "
                 f"{st.get('fill_s', 0.0):.3f}; kernels {st.get('ms_total', 0.0):.3f} ms, passes {st.get('ms_pass', 0.0):.3f} ms, finish "
                 f"{st.get('ms_finish', 0.0):.3f} ms)")
        if self.metric in _metrics.PARITY_NOTE:
            log.info(f"parity: {_metrics.parity_note(self.metric)}")
        self._distribution_files(found.inverted(), self.outdir, thresholds)
        return found

    # 4d, --distribution
    def cluster_distribution(self, groups, matrix, thresholds, clu_distance):
        """The distribution split by the final clusters (``groups`` as ``cluster_table`` takes them) into the staging directory.  On
        the dense route it is read off the matrix the run holds (``PairDistribution.from_dense``); on the --no-matrix route one
        distribution fill runs on the upload that route holds.  Integers either way: the files are the same on both."""
        self.banner("4d", f"{self.metric} pair distribution within and between the clusters")
        t0 = time.perf_counter()
        if matrix is not None:
            found = PairDistribution.from_dense(matrix, groups)
            how = "the dense matrix"
        else:
            ctx, metric, genome_names = self.fills
            index = {name: k for k, name in enumerate(genome_names)}
            label = np.zeros(len(genome_names), dtype=np.int32)
            for k, group in enumerate(groups):
                label[[index[name] for name in group]] = k
            hist, st = ctx.fill_hist(metric, label, len(groups), as_distance=True, want_stats=True)
            found = PairDistribution.from_hist(hist, is_distance=True, nodes=genome_names)
            how = f"{st.get('n_slabs', 1)} slab(s) of a distribution fill (passes {st.get('ms_pass', 0.0):.3f} ms)"
        log.info(f"{found.n_pairs:,} pairs, {found.within.n_pairs:,} of them inside the {len(groups):,} clusters and singletons, from {how} in "
                 f"{time.perf_counter() - t0:.3f} s")
        self._distribution_files(found.inverted(), self.stage, thresholds, clu_similarity=round(1.0 - clu_distance, 6))
        return found

    # 5 + 6
    def finish(self, matrix, multi, single, clu_distance, rm_tmp):
        self.banner(5, "dataset outputs")
        matrix.reorder([n for m in multi for n in m.nodes] + [n for m in single for n in m.nodes])
        matrix.invert()
        if len(matrix) > 1500:
            log.info("matrix too large for a dataset heatmap")
        else:
            for suffix in ("html", "svg"):
                draw_heatmap(matrix, colors=self.colors, midpoint=1.0 - clu_distance,
                             filename=self.stage / f"{self.metric}_heatmap.{suffix}")
        for old in self.outdir.iterdir():                      # clear earlier results, keep cache and log
            if old.name == self.cache.name or old.suffix == ".log":
                continue
            shutil.rmtree(old) if old.is_dir() else old.unlink()
        matrix_to_squareform(matrix, self.outdir / f"pairwise_{self.metric}_similarities.tsv")
        matrix_to_adjacency(matrix, self.outdir / f"pairwise_{self.metric}_adjacency.tsv", skip_zero=True)
        for name, other in self.also_matrices.items():         # --also: the same square under each further metric, in the same node order
            other.reorder(list(matrix.nodes))
            other.invert()
            matrix_to_squareform(other, self.outdir / f"pairwise_{name}_similarities.tsv")
        shutil.copytree(self.stage, self.outdir, dirs_exist_ok=True)
        shutil.rmtree(self.stage)
        if rm_tmp:
            shutil.rmtree(self.cache)


    # 5 + 6, --no-matrix
    def finish_no_matrix(self, rm_tmp):
        self.banner(5, "dataset outputs")
        log.info(f"--no-matrix: pairwise_{self.metric}_similarities.tsv and the dataset heatmap need the dense matrix and are not written; "
                 f"the adjacency file comes from an edge-list fill")
        for old in self.outdir.iterdir():                      # clear earlier results, keep cache and log
            if old.name == self.cache.name or old.suffix == ".log":
                continue
            shutil.rmtree(old) if old.is_dir() else old.unlink()
        ctx, metric, names = self.fills                        # the upload of clusters_no_matrix: the run's only one
        src, tgt, val, st = ctx.fill_edges(metric, 0.999999, as_distance=True, want_stats=True)    # 6-place values: d <= 0.999999 is sim > 0
        edges = SparseEdges(names, src, tgt, val, is_distance=True, threshold=0.999999)
        log.info(f"{len(edges):,} pairs of non-zero similarity from {st.get('n_slabs', 1)} slab(s) of the edge-list fill")
        edges_to_adjacency(edges.inverted(), self.outdir / f"pairwise_{self.metric}_adjacency.tsv", skip_zero=True)
        shutil.copytree(self.stage, self.outdir, dirs_exist_ok=True)
        shutil.rmtree(self.stage)
        if rm_tmp:
            shutil.rmtree(self.cache)


def phamclust(infile, outdir, is_genome_dir, metric, nr_distance, nr_linkage, clu_distance, clu_linkage, sub_distance,
              sub_linkage, k_min, no_sub, colors, midpoint, cpus, rm_tmp, debug, extend=None, adjacency_only=False, edge_thresh=None,
              components_only=False, no_matrix=False, tree=False, grow=None, cluster_table=False, cluster_fit=False, place=None, grow_table=None, join_min=None,
              distribution_only=False, distribution=False, pairs=None, prefilter=False, nearest_bound=False, also=None, grow_nearest=None, nearest=None):
    """Same signature as the reference's ``phamclust()`` (distances, not similarities, for the thresholds); ``extend``: the
    distance matrix of an earlier run over a subset of the genomes (``--extend``), or None; ``adjacency_only``: stop after an
    edge-list fill of the pairs of similarity >= ``edge_thresh`` (None: every non-zero one) and write only the adjacency file;
    ``components_only``: stop after a components fill -- genomes joined when distance < round(1 - ``edge_thresh``, 6), None: 0.0 --
    and write only ``components_<metric>.tsv``; ``no_matrix``: stages 2-3 from components and groups fills, without the dense matrix
    (same clusters; no similarities file, no dataset heatmap, no matrix cache; the adjacency file from an edge-list fill);
    ``nearest``: stop after a nearest-neighbours fill of that many neighbours per genome and write only ``nearest_<metric>.tsv``;
    ``tree``: stop after a tree fill and write only ``tree_<metric>.tsv``, the single-linkage dendrogram's edges in merge order;
    ``grow``: with ``tree``, the ``tree_<metric>.tsv`` -- with ``components_only`` and an ``edge_thresh``, the ``components_<metric>.tsv`` --
    an earlier run wrote over a subset of the genomes (``--grow``): only the pairs of the genomes it lacks are filled, on one GPU;
    ``grow_nearest``: with ``nearest``, the ``nearest_<metric>.tsv`` of an earlier run over a subset of the genomes (``--grow-nearest``),
    grown the same way; ``cluster_table``: after the clustering, one between-groups fill over the final clusters and its three outputs
    (``--cluster-table``; with the whole pipeline only, on either route); ``cluster_fit``: after the clustering, one affinity fill over the
    final clusters and its two files (``--cluster-fit``; on the same terms); ``place``: stop after placing the genomes that a
    ``cluster_fit_<metric>.tsv`` of an earlier run lacks against its clusters, and write only ``placement_<metric>.tsv`` (``--place``);
    ``grow_table``: with ``place``, the ``cluster_table_<metric>.tsv`` of the run that wrote that file: every new genome joins its nearest
    cluster by mean -- with ``join_min``, a similarity, only when that mean reaches it, else it becomes a singleton group -- and the
    table is grown by the new genomes' pairs alone (``--grow-table``, ``--join-min``); ``distribution_only``: stop after a distribution fill and
    write only the histogram of all pair similarities and its summary (``--distribution-only``; ``edge_thresh`` then adds a line to the
    summary); ``distribution``: after the clustering, the same two files split by the final clusters (``--distribution``; with the whole
    pipeline only, on either route); ``pairs``: stop after a pair-list fill of the pairs that file names and write only
    ``pairwise_<metric>_pairs.tsv`` (``--pairs``); ``prefilter``: with ``adjacency_only``, peq and an ``edge_thresh``, the same adjacency
    file from the af edge list's pairs alone (``--prefilter``); ``nearest_bound``: with ``nearest`` and peq, the same lists from the
    pairs the af bound leaves open (``--af-bound``); ``also``: further metric names beside ``metric``, filled off the same alignment pass
    (``--also``): on the dense route each is cached and written as ``pairwise_<name>_similarities.tsv`` while the clustering runs on
    ``metric``'s matrix alone; with ``pairs`` one ``pairwise_<name>_pairs.tsv`` each."""
    also = list(also or [])
    if also:
        if any(name not in METRICS for name in also) or metric in also or len(set(also)) != len(also):
            raise ValueError(f"also names metrics among {', '.join(METRICS)} beside '{metric}', each once")
        if (adjacency_only or components_only or no_matrix or tree or nearest is not None or extend is not None or grow is not None or
                grow_nearest is not None or place is not None or distribution_only or prefilter or nearest_bound):
            raise ValueError("also goes with the dense route or with pairs; it cannot be combined with adjacency_only, components_only, no_matrix, "
                             "tree, nearest, extend, grow, grow_nearest, place, distribution_only, prefilter or nearest_bound")
    if pairs is not None and (adjacency_only or components_only or no_matrix or tree or nearest is not None or extend is not None or grow is not None or
                              place is not None or cluster_table or cluster_fit or distribution or distribution_only or prefilter):
        raise ValueError("pairs cannot be combined with adjacency_only, components_only, no_matrix, tree, nearest, extend, grow, place, cluster_table, "
                         "cluster_fit, distribution, distribution_only or prefilter")
    if prefilter and not (adjacency_only and metric == "peq" and edge_thresh is not None):
        raise ValueError("prefilter goes with adjacency_only, the peq metric and an edge_thresh")
    if nearest_bound and not (nearest is not None and metric == "peq" and grow_nearest is None):
        raise ValueError("nearest_bound goes with nearest and the peq metric, and not with grow_nearest")
    if distribution_only and (adjacency_only or components_only or no_matrix or tree or nearest is not None or extend is not None or grow is not None or
                              place is not None or cluster_table or cluster_fit or distribution):
        raise ValueError("distribution_only cannot be combined with adjacency_only, components_only, no_matrix, tree, nearest, extend, grow, place, "
                         "cluster_table, cluster_fit or distribution")
    if distribution and (adjacency_only or components_only or tree or nearest is not None or extend is not None or place is not None):
        raise ValueError("distribution cannot be combined with adjacency_only, components_only, tree, nearest, extend or place")
    if grow_table is not None and place is None:
        raise ValueError("grow_table goes with place")
    if join_min is not None and grow_table is None:
        raise ValueError("join_min goes with grow_table")
    if place is not None and (adjacency_only or components_only or no_matrix or tree or nearest is not None or extend is not None or grow is not None or
                              grow_nearest is not None or cluster_table or cluster_fit):
        raise ValueError("place cannot be combined with adjacency_only, components_only, no_matrix, tree, nearest, extend, grow, cluster_table or cluster_fit")
    if cluster_fit and (adjacency_only or components_only or tree or nearest is not None or extend is not None):
        raise ValueError("cluster_fit cannot be combined with adjacency_only, components_only, tree, nearest or extend")
    if cluster_table and (adjacency_only or components_only or tree or nearest is not None or extend is not None):
        raise ValueError("cluster_table cannot be combined with adjacency_only, components_only, tree, nearest or extend")
    if grow_nearest is not None and (nearest is None or grow is not None):
        raise ValueError("grow_nearest goes with nearest, and not with grow")
    if grow is not None:
        if adjacency_only or no_matrix or nearest is not None or extend is not None or tree == bool(components_only):
            raise ValueError("grow goes with exactly one of tree and components_only, and with nothing else")
        if components_only and edge_thresh is None:
            raise ValueError("grow with components_only needs the edge_thresh the stored components were filled at")
    if tree and (adjacency_only or components_only or no_matrix or nearest is not None or extend is not None):
        raise ValueError("tree cannot be combined with adjacency_only, components_only, no_matrix, nearest or extend")
    if nearest is not None:
        if isinstance(nearest, bool) or not isinstance(nearest, int) or not 1 <= nearest <= _matrix.NEAREST_MAX_K:
            raise ValueError(f"nearest is a number of neighbours in 1..{_matrix.NEAREST_MAX_K}")
        if adjacency_only or components_only or no_matrix or extend is not None:
            raise ValueError("nearest cannot be combined with adjacency_only, components_only, no_matrix or extend")
    if no_matrix and (adjacency_only or components_only or extend is not None):
        raise ValueError("no-matrix cannot be combined with adjacency_only, components_only or extend")
    if no_matrix and "ward" in (nr_linkage, clu_linkage):
        raise ValueError("no-matrix: ward's clusters can span components; the nr and clu passes take single, average or complete")
    if adjacency_only and extend is not None:
        raise ValueError("adjacency_only cannot be combined with extend")
    if components_only and (adjacency_only or extend is not None):
        raise ValueError("components_only cannot be combined with adjacency_only or extend")
    if edge_thresh is not None and not (adjacency_only or components_only or distribution_only):
        raise ValueError("edge_thresh selects the edges of adjacency_only or components_only")
    if nr_distance >= clu_distance:          # pre-grouping must be tighter than clustering, else switch it off
        nr_distance = 0.0
    settings = dict(infile=infile, outdir=outdir, metric=metric, nr=(nr_distance, nr_linkage), clu=(clu_distance, clu_linkage),
                    sub=(sub_distance, sub_linkage), k_min=k_min, subcluster=not no_sub, colors=",".join(colors),
                    midpoint=midpoint, cpus=cpus, remove_tmp=rm_tmp, debug=debug)
    if extend is not None:
        settings["extend"] = extend
    if adjacency_only:
        settings["adjacency"] = "only" + ("" if edge_thresh is None else f", similarity >= {edge_thresh}") + (" (--prefilter: behind the af bound)" if prefilter else "")
    if pairs is not None:
        settings["pairs"] = f"only, the pairs listed in {pairs}"
    if also:
        settings["also"] = f"{', '.join(also)} (--also: off the same alignment pass)"
    if no_matrix:
        settings["matrix"] = "none (--no-matrix: components and groups fills)"
    if components_only:
        settings["components"] = f"only, joined at similarity > {0.0 if edge_thresh is None else edge_thresh}"
    if nearest is not None:
        settings["nearest"] = f"only, {nearest} neighbours per genome" + (" (--af-bound: behind the af bound)" if nearest_bound else "")
    if tree:
        settings["tree"] = "only (single-linkage dendrogram)"
    if distribution_only:
        settings["histogram"] = "only (--distribution-only: the distribution of all pair similarities)"
    if distribution:
        settings["histogram"] = "written, within and between the clusters (--distribution)"
    if cluster_table:
        settings["clusters"] = "with their table (--cluster-table: a between-groups fill)"
    if cluster_fit:
        settings["cluster fit"] = "written (--cluster-fit: an affinity fill)"
    if place is not None:
        settings["place"] = f"only, against the clusters of {place}"
    if grow_table is not None:
        settings["table"] = f"{grow_table}, grown by the placed genomes" + ("" if join_min is None else f" (joining at similarity >= {join_min})")
    if grow is not None:
        settings["grow"] = grow
    if grow_nearest is not None:
        settings["grow"] = grow_nearest
    log.info("--- 0: settings ---")
    for key, value in settings.items():
        log.info(f"{key:<11}{value}")
    run = _Run(outdir, metric, colors, midpoint)
    run.extend = extend
    run.grow = grow
    run.grow_nearest = grow_nearest
    run.also = also
    run.rank, run.world = distributed.ensure_process_group()      # (0, 1) unless started by torch.distributed.run
    _mark("torch_import_and_process_group")
    run.read(infile, is_genome_dir)
    if adjacency_only:
        if run.world > 1:
            log.error("--adjacency-only is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        run.adjacency(edge_thresh, prefilter=prefilter)
        run.banner(3, "done (--adjacency-only: no clustering)")
        return
    if pairs is not None:
        if run.world > 1:
            log.error("--pairs is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        run.pairs(pairs)
        run.banner(3, "done (--pairs: no clustering)")
        return
    if components_only:
        if run.world > 1:
            log.error("--components-only is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        run.components(0.0 if edge_thresh is None else edge_thresh)
        run.banner(3, "done (--components-only: no clustering)")
        return
    if nearest is not None:
        if run.world > 1:
            log.error("--nearest is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        run.nearest(nearest, bound=nearest_bound)
        run.banner(3, "done (--nearest: no clustering)")
        return
    if place is not None:
        if run.world > 1:
            log.error("--place is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        found = run.place(place)
        if grow_table is not None:
            run.grow_table(place, grow_table, found, join_min)
        run.banner(3, "done (--place: no clustering)")
        return
    if tree:
        if run.world > 1:
            log.error("--tree is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        run.tree()
        run.banner(3, "done (--tree: no clustering)")
        return
    as_similarity = lambda distance: round(1.0 - distance, 6)          # noqa: E731
    thresholds = [("nr_thresh", as_similarity(nr_distance)), ("clu_thresh", as_similarity(clu_distance)), ("sub_thresh", as_similarity(sub_distance))]
    if distribution_only:
        if run.world > 1:
            log.error("--distribution-only is a one-process call: run it in one process, not under a launcher")
            sys.exit(1)
        run.distribution(thresholds + ([] if edge_thresh is None else [("edge_thresh", edge_thresh)]))
        run.banner(3, "done (--distribution-only: no clustering)")
        return
    if distribution and run.world > 1:
        log.error("--distribution is a one-process call: run it in one process, not under a launcher")
        sys.exit(1)
    if cluster_table and run.world > 1:
        log.error("--cluster-table is a one-process call: run it in one process, not under a launcher")
        sys.exit(1)
    if cluster_fit and run.world > 1:
        log.error("--cluster-fit is a one-process call: run it in one process, not under a launcher")
        sys.exit(1)
    matrix = None
    if no_matrix:
        if run.world > 1:
            log.error("--no-matrix runs on one GPU: run it in one process, not under a launcher")
            sys.exit(1)
        multi, single = run.clusters_no_matrix((nr_distance, nr_linkage), (clu_distance, clu_linkage))
    else:
        if also and run.world > 1:
            log.error("--also is a one-GPU call: run it in one process, not under a launcher")
            sys.exit(1)
        matrix = run.distances_also(cpus) if also else run.distances(cpus)
        if matrix is None:                    # ranks other than 0 are done once their shard is gathered
            return
        multi, single = run.clusters(matrix, (nr_distance, nr_linkage), (clu_distance, clu_linkage))
    final_groups = [list(m.nodes) for m in multi] + [list(m.nodes) for m in single]
    run.banner(4, "sub-clusters")
    run.stage = run._dir(run.cache / "03_clusters")
    for number, cluster in enumerate(multi, start=1):
        log.info(f"cluster {number}: {len(cluster)} genomes")
        run.write_cluster(number, cluster, (sub_distance, sub_linkage), k_min, no_sub)
    if single:
        lone = run._dir(run._dir(run.stage / "singletons", fresh=True) / "genomes")
        for one in single:
            name = one.nodes[0]
            run.by_name[name].save(lone / f"{name}.faa")
    if cluster_table:
        run.cluster_table(final_groups, clu_distance)
    if cluster_fit:
        run.cluster_fit(final_groups)
    if distribution:
        run.cluster_distribution(final_groups, matrix, thresholds, clu_distance)
    if no_matrix:
        run.finish_no_matrix(rm_tmp)
    else:
        run.finish(matrix, multi, single, clu_distance, rm_tmp)


def _colors(text):
    colors = text.split(",")
    if not 2 <= len(colors) <= 3:
        log.error(f"expected either two or three colors, got {len(colors)}")
        sys.exit(1)
    bad = [c for c in colors if c not in CSS_COLORS]
    if bad:
        log.error(f"unknown colors {bad}; valid colors: {' '.join(sorted(CSS_COLORS))}")
        sys.exit(1)
    if len(colors) == 2:
        log.warning("2-color scale ignores `--heatmap-midpoint`")
    return colors


SLAB_FILL_FLAGS = (("adjacency_only", "--adjacency-only", "fills an edge list"), ("components_only", "--components-only", "fills component labels"),
                   ("nearest", "--nearest", "fills nearest-neighbour lists"), ("tree", "--tree", "fills the single-linkage tree"),
                   ("distribution_only", "--distribution-only", "fills the pair distribution"))


def gpus_plan(args, route, packed):
    """What ``--gpus N`` (N > 1, one process, no launcher around it) comes to: ``(n_gpus, how, note)`` with ``how`` "process" (this
    process drives n_gpus devices: PHAMCLUST_GPUS), "launcher" (n_gpus ranks are started) or "one" (the matrix stage stays on one
    GPU; ``note`` says why).  Host arithmetic on the parsed arguments and the packed genomes (None: no estimate) -- no GPU call.
    --extend's rows fill is a one-GPU call.  --adjacency-only, --components-only, --nearest and --tree spread over the GPUs of this process
    (pc_multi_fill_edges / _components / _nearest / _tree) under the same estimate as the dense fill; one process per GPU has no route for
    them, so under PHAMCLUST_MULTI=launcher they stay on one GPU."""
    if getattr(args, "grow_nearest", None) is not None:
        return 1, "one", "--grow-nearest fills only the pairs of the new genomes, which is a one-GPU call: the matrix stage stays on one GPU"
    if getattr(args, "place", None) is not None:
        return 1, "one", "--place fills only the pairs of the new genomes, which is a one-GPU call: the matrix stage stays on one GPU"
    if getattr(args, "grow", None) is not None:
        return 1, "one", "--grow fills only the pairs of the new genomes, which is a one-GPU call: the matrix stage stays on one GPU"
    if args.extend is not None:
        # (pc_fill_rows refuses a sharded context): the matrix stage stays in this process, on one GPU
        return 1, "one", "--extend fills only the new genomes' rows, which is a one-GPU call: the matrix stage stays on one GPU"
    if route == "launcher" and getattr(args, "cluster_table", False):
        return 1, "one", "--cluster-table fills the clusters' table from one process: the matrix stage stays on one GPU"
    if route == "launcher" and getattr(args, "distribution", False):
        return 1, "one", "--distribution reads the clusters' pair distribution from one process: the matrix stage stays on one GPU"
    if route == "launcher" and getattr(args, "cluster_fit", False):
        return 1, "one", "--cluster-fit fills the genomes' affinity to the clusters from one process: the matrix stage stays on one GPU"
    if route == "launcher":
        for attr, flag, what in SLAB_FILL_FLAGS:
            if getattr(args, attr) not in (None, False):
                return 1, "one", f"{flag} {what}, which is a one-GPU call: the matrix stage stays on one GPU"
    n_gpus, note = args.gpus, None
    if packed is not None:
        n_gpus, note = startup.choose_gpus(args.gpus, packed, args.metric, route)
    if n_gpus > 1 and route == "launcher":
        return n_gpus, "launcher", note
    if n_gpus > 1:
        if args.device is not None:
            note = (note or "") + (f"; --device {args.device} is IGNORED: {n_gpus} GPUs from one process are devices 0..{n_gpus - 1} "
                                   f"(name others with PHAMCLUST_GPU_IDS)")
        return n_gpus, "process", note
    return 1, "one", note


def main(argv=None):
    if argv is None and len(sys.argv) == 1:
        sys.argv.append("-h")
    args = parse_args(argv)
    if not (args.infile.is_dir() if args.genome_dir else args.infile.is_file()):
        kind = "genome directory" if args.genome_dir else "input TSV"
        print(f"{kind} '{args.infile}' does not exist")
        sys.exit(1)
    global TIMELINE
    TIMELINE = startup.Timeline()
    TIMELINE.mark("imports")
    # What this run tells the library layers through the environment (PHAMCLUST_GPUS / _NO_TORCH / _DEVICE) is THIS RUN's: the old
    # values come back when main() returns, so that a caller of main() -- a test, a notebook -- does not find its later
    # matrix_de_novo calls redirected to N GPUs, or its later `import torch` next to a HIP runtime bound without it.
    saved_env = {key: os.environ.get(key) for key in ("PHAMCLUST_GPUS", "PHAMCLUST_GPU_IDS", "PHAMCLUST_NO_TORCH", "PHAMCLUST_DEVICE")}
    try:
        _run(args, argv)
    finally:
        for key, value in saved_env.items():
            if value is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = value


def _run(args, argv):
    rank, _, world = distributed.env_world()
    gpus_note = None
    if args.gpus > 1 and world == 1:
        # `--gpus N`.  Two routes (startup.multi_gpu_route): by default THIS process drives the N GPUs (pc_multi_*: nothing to
        # launch); PHAMCLUST_MULTI=launcher re-runs the command as N ranks under torch.distributed.run, which costs seconds
        # before the first pair (an interpreter, a torch import and a process group per rank).  Either way the reference's rule
        # applies -- never more workers than work (matrix.py:460-462): load the genomes (host code only, no GPU call), estimate
        # the fill, and spread it only when N GPUs can win their start-up back (gpus_plan).
        route = startup.multi_gpu_route()
        packed = None
        if not args.genome_dir and gpus_plan(args, route, None)[0] > 1:
            genomes = load_genomes(args.infile)
            TIMELINE.mark("load_genomes_for_estimate")
            packed = packed_behind(genomes)
            if packed is not None:
                _PRELOADED[str(args.infile)] = genomes
        n_gpus, how, gpus_note = gpus_plan(args, route, packed)
        if how == "launcher":
            # as N ranks, one per GPU -- as a child process, before this process has made a single GPU call
            passed = list(sys.argv[1:] if argv is None else argv)
            sys.exit(distributed.launch_ranks(n_gpus, "phamclust_amd", [str(x) for x in passed],
                                              env={"PHAMCLUST_T0": repr(TIMELINE.t_launch), "PHAMCLUST_FORCE_GPUS": "1"}))
        if how == "process":
            os.environ["PHAMCLUST_GPUS"] = str(n_gpus)             # matrix_de_novo and the edge / components / nearest fills: devices 0..N-1 from this process (PHAMCLUST_GPU_IDS names others)
        else:
            os.environ.pop("PHAMCLUST_GPUS", None); os.environ.pop("PHAMCLUST_GPU_IDS", None)
    if world == 1:
        os.environ.setdefault("PHAMCLUST_NO_TORCH", "1")           # one rank: nothing needs torch (hip.load() then skips its import)
    if args.device is not None and world == 1:
        os.environ["PHAMCLUST_DEVICE"] = str(args.device)           # matrix.default_device reads it when the context is made
    args.outdir.mkdir(parents=True, exist_ok=True)
    if rank == 0:
        logging.basicConfig(filename=args.outdir / "phamclust.log", filemode="w", format=LOG_STR_FMT, datefmt=LOG_TIME_FMT,
                            level=logging.DEBUG if args.debug else logging.INFO, force=True)
        log.addHandler(logging.StreamHandler(sys.stdout))
    else:                                     # rank 0 owns the log file and the output tree
        logging.basicConfig(stream=sys.stderr, format=f"phamclust[rank {rank}]: %(levelname)s: %(message)s", level=logging.WARNING, force=True)
    if gpus_note and rank == 0:
        log.info(f"--gpus {args.gpus}: {gpus_note}")
    as_distance = lambda similarity: round(1.0 - similarity, 6)          # noqa: E731
    try:
        phamclust(infile=args.infile, outdir=args.outdir, is_genome_dir=args.genome_dir, metric=args.metric,
                  nr_distance=as_distance(args.nr_thresh), nr_linkage=args.nr_linkage,
                  clu_distance=as_distance(args.clu_thresh), clu_linkage=args.clu_linkage,
                  sub_distance=as_distance(args.sub_thresh), sub_linkage=args.sub_linkage, k_min=max(1, args.k_min),
                  no_sub=args.no_sub, colors=_colors(args.heatmap_colors), midpoint=round(args.heatmap_midpoint, 6),
                  cpus=args.threads, rm_tmp=args.remove_tmp, debug=args.debug, extend=args.extend,
                  adjacency_only=args.adjacency_only, edge_thresh=args.edge_thresh, components_only=args.components_only, no_matrix=args.no_matrix,
                  nearest=args.nearest, tree=args.tree, grow=args.grow, grow_nearest=args.grow_nearest, cluster_table=args.cluster_table,
                  cluster_fit=args.cluster_fit, place=args.place, grow_table=args.grow_table, join_min=args.join_min,
                  distribution_only=args.distribution_only, distribution=args.distribution, pairs=args.pairs, prefilter=args.prefilter, nearest_bound=args.af_bound,
                  also=args.also)
    finally:
        if rank == 0:
            TIMELINE.mark("clustering_and_outputs")
            log.info(TIMELINE.line())
        if world > 1:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()


if __name__ == "__main__":
    main()
