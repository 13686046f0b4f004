"""Command line of the pipeline: same flags, defaults and ``METRICS`` selector as the reference
(cli.py:10-117), declared here as a table so that the defaults are inspectable (``DEFAULTS``)."""

import argparse
import os
import pathlib
from multiprocessing import cpu_count

from phamclust_amd import metrics as _m
from phamclust_amd.metrics import *          # noqa: F401,F403  re-export the six metric callables

# name -> callable, in the reference's order; `-m` picks one of these keys
METRICS = dict(gcs=_m.gene_content_similarity, jc=_m.jaccard_coefficient, pocp=_m.percentage_of_conserved_proteins,
               af=_m.alignment_fraction, aai=_m.average_aminoacid_identity, peq=_m.proteomic_equivalence_quotient)
LINKAGES = {"single", "average", "complete"}
CPUS = cpu_count()
GPUS = 1                                     # the fill's counterpart of -t: how many GPUs share the pair list
COLORS = "red,yellow,green"
METRIC, K_MIN = "peq", 6
NR_THRESH, NR_LINKAGE = 0.75, "complete"     # 1st pass: glue near-identical genomes together
CLU_THRESH, CLU_LINKAGE = 0.25, "average"    # 2nd pass: clusters
SUB_THRESH, SUB_LINKAGE = 0.6, "single"      # 3rd pass: sub-clusters
NEAREST_MAX_K = 64                           # --nearest: the k a nearest-neighbours fill takes at most (PC_NEAREST_MAX_K)

_PAPERS = (("gcs", "gene content similarity", "10.1038/nmicrobiol.2017.112"),
           ("jc", "jaccard coefficient", "10.1111/j.1469-8137.1912.tb05611.x"),
           ("pocp", "percentage of conserved proteins", "10.1128/JB.01688-14"),
           ("af", "alignment fraction", "10.1093/nar/gkv657"),
           ("aai", "average aminoacid identity", "10.1073/pnas.0409727102"),
           ("peq", "proteomic equivalence quotient", "10.1128/msystems.00443-23"))
EPILOG = "\nAvailable metrics:\n\n" + "\n".join(
    f"({i}) {key:<6}{title:<36}https://doi.org/{doi}" for i, (key, title, doi) in enumerate(_PAPERS, start=1)) + "\n"

# (group, short, long, kwargs); "%(default)s" is filled in by argparse
_OPTIONS = (
    (None, "-g", "--genome-dir", dict(action="store_true", help="`infile` is a directory with one FASTA per genome, not a TSV")),
    ("clustering arguments:", "-k", "--k-min", dict(type=int, default=K_MIN, help="smallest cluster that gets sub-clustered")),
    ("clustering arguments:", "-s", "--sub-thresh", dict(type=float, default=SUB_THRESH, help="similarity threshold of the sub-clustering pass")),
    ("clustering arguments:", "-sl", "--sub-linkage", dict(type=str, choices=LINKAGES, default=SUB_LINKAGE, help="linkage of the sub-clustering pass")),
    ("clustering arguments:", "-c", "--clu-thresh", dict(type=float, default=CLU_THRESH, help="similarity threshold of the clustering pass")),
    ("clustering arguments:", "-cl", "--clu-linkage", dict(type=str, choices=LINKAGES, default=CLU_LINKAGE, help="linkage of the clustering pass")),
    ("clustering arguments:", "-nr", "--nr-thresh", dict(type=float, default=NR_THRESH, help="similarity above which genomes are pre-grouped and can never be split")),
    ("clustering arguments:", "-nl", "--nr-linkage", dict(type=str, choices=LINKAGES, default=NR_LINKAGE, help="linkage of that pre-grouping pass")),
    ("clustering arguments:", "-m", "--metric", dict(type=str, choices=METRICS, default=METRIC, help="pairwise relatedness index (see below)")),
    ("heatmap arguments:", "-hc", "--heatmap-colors", dict(type=str, default=COLORS, help="2 or 3 comma-separated CSS colour names")),
    ("heatmap arguments:", "-hm", "--heatmap-midpoint", dict(type=float, default=0.5, help="where the middle colour sits on a 3-colour scale")),
    (None, "-d", "--debug", dict(action="store_true", help="log at DEBUG level")),
    (None, "-n", "--no-sub", dict(action="store_true", help="skip the sub-clustering pass")),
    (None, "-r", "--remove-tmp", dict(action="store_true", help="delete the cache directory at the end (re-runs then recompute the matrix)")),
    (None, "-x", "--extend", dict(type=pathlib.Path, default=None, help="distance matrix an earlier run wrote over a SUBSET of these genomes (its cache's "
                                                                       "02_distmats/<metric>_distance_matrix.tsv, or a squareform file): only the rows "
                                                                       "of the genomes it lacks are filled, on one GPU")),
    (None, "-A", "--adjacency-only", dict(action="store_true", help="stop after the matrix stage and write only pairwise_<metric>_adjacency.tsv, from an "
                                                                    "edge-list fill: the dense matrix is neither delivered nor cached, and no clustering runs; "
                                                                    "with --gpus N the fill is spread over N GPUs of this process")),
    (None, "-C", "--components-only", dict(action="store_true", help="stop after the matrix stage and write only components_<metric>.tsv, from a "
                                                                     "components fill: the single-linkage groups at --edge-thresh (genomes joined "
                                                                     "when distance < 1 - SIM); no matrix, no edge list, no clustering; with --gpus N "
                                                                     "the fill is spread over N GPUs of this process")),
    (None, "-N", "--no-matrix", dict(action="store_true", help="cluster without the dense matrix: components fills find the groups, groups fills "
                                                               "their sub-matrices (sum of n_c^2 cells, not N^2); same cluster_* / singletons "
                                                               "output; the adjacency file comes from an edge-list fill; no "
                                                               "pairwise_<metric>_similarities.tsv, no dataset heatmap, no matrix cache; one GPU")),
    (None, "-K", "--nearest", dict(type=int, default=None, help="stop after the matrix stage and write only nearest_<metric>.tsv, from a nearest-neighbours "
                                                               "fill: each genome's K most similar genomes (1..64), most similar first; no matrix, "
                                                               "no threshold, no clustering; with --gpus N the fill is spread over N GPUs of this process")),
    (None, "-T", "--tree", dict(action="store_true", help="stop after the matrix stage and write only tree_<metric>.tsv, from a tree fill: the "
                                                          "single-linkage dendrogram as N-1 lines source<TAB>target<TAB>similarity in merge "
                                                          "order, from which the clusters at every threshold follow; no matrix, no threshold, no "
                                                          "clustering; with --gpus N the devices of this process share the fill")),
    (None, "-w", "--grow", dict(type=pathlib.Path, default=None, help="with --tree: the tree_<metric>.tsv, with --components-only --edge-thresh SIM: the "
                                                                     "components_<metric>.tsv an earlier run wrote over a SUBSET of these genomes: only "
                                                                     "the pairs of the genomes it lacks are filled, on one GPU, and the file written is "
                                                                     "the from-scratch run's, byte for byte; the adjacency file has no such route (it "
                                                                     "does not say which genomes it covered: matrix.edges_extend is the API for it)")),
    (None, "-W", "--grow-nearest", dict(type=pathlib.Path, default=None, help="with --nearest K: the nearest_<metric>.tsv an earlier --nearest run (of at "
                                                                             "least K neighbours) wrote over a SUBSET of these genomes: only the pairs "
                                                                             "of the genomes it lacks are filled, on one GPU, and the file written is "
                                                                             "the from-scratch run's, byte for byte")),
    (None, "-B", "--cluster-table", dict(action="store_true", help="after clustering, one between-groups fill over the final clusters (the "
                                                                   "multi-genome clusters in output order, then the singletons): writes "
                                                                   "cluster_table_<metric>.tsv (count, mean, min, max similarity of every two "
                                                                   "clusters), cluster_<metric>_similarities.tsv (their mean similarity as a "
                                                                   "square) and, for at most 1500 clusters, cluster_<metric>_heatmap.{html,svg}; "
                                                                   "with the dense route or --no-matrix, and with --gpus N")),
    (None, "-F", "--cluster-fit", dict(action="store_true", help="after clustering, one affinity fill over the final clusters (as "
                                                                 "--cluster-table takes them): writes cluster_fit_<metric>.tsv (per genome: its "
                                                                 "cluster, mean similarity to it, the nearest other cluster and that mean, its "
                                                                 "silhouette, whether it is the cluster's medoid) and "
                                                                 "cluster_fit_<metric>_summary.tsv (per cluster: size, medoid, mean silhouette, "
                                                                 "largest own distance); with the dense route or --no-matrix, and with --gpus N")),
    (None, "-H", "--distribution-only", dict(action="store_true", help="stop after the matrix stage and write only pairwise_<metric>_distribution.tsv (the "
                                                                       "exact histogram of all pair similarities: value<TAB>count per occupied "
                                                                       "millionth) and pairwise_<metric>_distribution_summary.tsv (n, min, max, mean, "
                                                                       "std, skew, quartiles, and how many pairs pass --nr-thresh, --clu-thresh, "
                                                                       "--sub-thresh and --edge-thresh), from a distribution fill: no matrix, no "
                                                                       "threshold, no clustering; with --gpus N the devices of this process share the fill")),
    (None, "-U", "--distribution", dict(action="store_true", help="after clustering, the distribution of the pair similarities split by the final "
                                                                  "clusters: writes pairwise_<metric>_distribution.tsv (value<TAB>within<TAB>between) "
                                                                  "and pairwise_<metric>_distribution_summary.tsv, which also says how --clu-thresh "
                                                                  "separates the clusters and which threshold would separate them best; with the "
                                                                  "dense route or --no-matrix")),
    (None, "-P", "--place", dict(type=pathlib.Path, default=None, help="stop after the matrix stage and write only placement_<metric>.tsv: FILE is the "
                                                                      "cluster_fit_<metric>.tsv of an earlier --cluster-fit run over a SUBSET of "
                                                                      "these genomes; the genomes it lacks are placed against its clusters -- per new "
                                                                      "genome the nearest cluster by mean, by nearest and by farthest member, with the "
                                                                      "three similarities and the clusters' sizes -- filling only the new genomes' "
                                                                      "pairs, on one GPU; no matrix, no clustering")),
    (None, "-b", "--grow-table", dict(type=pathlib.Path, default=None, help="with --place FIT: FILE is the cluster_table_<metric>.tsv of the run that "
                                                                           "wrote FIT; after the placement every new genome joins its nearest cluster by "
                                                                           "mean and the stored table is grown by the new genomes' pairs alone (exact: "
                                                                           "counts and sums add, extremes only move outward); writes "
                                                                           "cluster_table_<metric>.tsv beside placement_<metric>.tsv")),
    (None, "-j", "--join-min", dict(type=float, default=None, help="with --grow-table: a new genome whose nearest mean similarity lies below SIM "
                                                                   "joins no cluster and becomes a singleton group of its own, appended after "
                                                                   "the stored groups in genome order")),
    (None, "-e", "--edge-thresh", dict(type=float, default=None, help="with --adjacency-only: keep the pairs of at least this similarity "
                                                                      "(default: every non-zero similarity, what the pipeline's file holds); with "
                                                                      "--components-only: join genomes of distance below 1 - this similarity "
                                                                      "(default 0.0: any non-zero similarity joins)")),
    (None, "-L", "--pairs", dict(type=pathlib.Path, default=None, help="stop after the matrix stage and write only pairwise_<metric>_pairs.tsv: FILE names "
                                                                      "one pair per line, two tab-separated genome names (further columns are ignored, "
                                                                      "so an adjacency file of any metric is valid input); the file written holds "
                                                                      "source<TAB>target<TAB>similarity in FILE's order, each pair oriented as written, "
                                                                      "from one pair-list fill on one GPU; nothing else is computed")),
    (None, "-O", "--also", dict(type=str, default=None, help="METRIC[,METRIC...]: further metrics beside -m's, off the same alignment pass (one joint "
                                                             "fill serves aai and peq together, and af / pocp / gcs / jc with them).  On the "
                                                             "dense route on one GPU: each metric's matrix is cached as -m's is and written as "
                                                             "pairwise_<metric>_similarities.tsv in the node order of -m's file; the clustering "
                                                             "runs on -m's matrix alone.  With --pairs FILE: one pairwise_<metric>_pairs.tsv per metric")),
    (None, "-f", "--prefilter", dict(action="store_true", help="with --adjacency-only -m peq --edge-thresh SIM: fill the af edge list at SIM first (peq "
                                                               "never exceeds af) and align only its pairs; the same file byte for byte, on one GPU")),
    (None, "-a", "--af-bound", dict(action="store_true", help="with --nearest K -m peq: seed every genome's list from its K nearest by af, then align "
                                                              "only the pairs whose af similarity can still reach the K-th value of either "
                                                              "genome (peq never exceeds af); the same file byte for byte, on one GPU; falls "
                                                              "back to the plain fill when more than half the pairs remain candidates; it "
                                                              "pays for small K and loses where K reaches the size of the clusters (README)")),
    (None, "-t", "--threads", dict(type=int, default=CPUS, help="accepted for compatibility; the six metrics run on the GPU (see --gpus)")),
    (None, "-D", "--device", dict(type=int, default=None, help="HIP device ordinal of a single-GPU run (default: PHAMCLUST_DEVICE, else 0); "
                                                               "with --gpus N the ranks take devices 0..N-1")),
    (None, "-G", "--gpus", dict(type=int, default=GPUS, help="GPUs of this node to spread the matrix fill over (one process per GPU "
                                                              "under torch.distributed.run, static pair shard, one RCCL gather); "
                                                              "--adjacency-only, --components-only, --nearest and --tree spread over them "
                                                              "from one process, a stretch of target genomes per GPU")),
)
DEFAULTS = {long.lstrip("-").replace("-", "_"): kw.get("default", False) for _, _, long, kw in _OPTIONS}


def build_parser():
    parser = argparse.ArgumentParser(prog="phamclust", epilog=EPILOG, formatter_class=argparse.RawTextHelpFormatter,
                                     description="Cluster phage genomes using gene content similarity-based metrics.")
    parser.add_argument("infile", type=pathlib.Path, help="TSV: genome <tab> pham <tab> translation (translation optional)")
    parser.add_argument("outdir", type=pathlib.Path, help="where results (and the cache directory) are written")
    groups = {}
    for group, short, long, kwargs in _OPTIONS:
        target = parser if group is None else groups.setdefault(group, parser.add_argument_group(group))
        kwargs = dict(kwargs)
        if "default" in kwargs:
            kwargs["help"] += " [default: %(default)s]"
            kwargs["metavar"] = ""
        target.add_argument(short, long, **kwargs)
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.edge_thresh is not None and not (args.adjacency_only or args.components_only or args.distribution_only):
        parser.error("--edge-thresh selects the edges of --adjacency-only or --components-only; without one of them there is nothing to select")
    if args.edge_thresh is not None and not 0.0 <= args.edge_thresh <= 1.0:          # (also refuses NaN)
        parser.error("--edge-thresh is a similarity in [0, 1]")
    if args.adjacency_only and args.extend is not None:
        parser.error("--adjacency-only fills an edge list from scratch; it cannot be combined with --extend")
    if args.components_only and args.adjacency_only:
        parser.error("--components-only and --adjacency-only each stop after a fill of their own; give one of them")
    if args.components_only and args.extend is not None:
        parser.error("--components-only fills from scratch; it cannot be combined with --extend")
    if args.nearest is not None:
        if not 1 <= args.nearest <= NEAREST_MAX_K:
            parser.error(f"--nearest takes a number of neighbours in 1..{NEAREST_MAX_K}")
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--no-matrix", args.no_matrix),
                            ("--extend", args.extend is not None)):
            if given:
                parser.error(f"--nearest stops after a nearest-neighbours fill of its own; it cannot be combined with {flag}")
    if args.tree:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--no-matrix", args.no_matrix),
                            ("--nearest", args.nearest is not None), ("--extend", args.extend is not None)):
            if given:
                parser.error(f"--tree stops after a tree fill of its own; it cannot be combined with {flag}")
    if args.distribution_only:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--no-matrix", args.no_matrix),
                            ("--nearest", args.nearest is not None), ("--tree", args.tree), ("--extend", args.extend is not None),
                            ("--grow", args.grow is not None), ("--place", args.place is not None), ("--cluster-table", args.cluster_table),
                            ("--cluster-fit", args.cluster_fit), ("--distribution", args.distribution)):
            if given:
                parser.error(f"--distribution-only stops after a distribution fill of its own; it cannot be combined with {flag}")
    if args.distribution:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--tree", args.tree),
                            ("--nearest", args.nearest is not None), ("--extend", args.extend is not None), ("--place", args.place is not None)):
            if given:
                parser.error(f"--distribution reads the final clusters of the whole pipeline; it cannot be combined with {flag}")
    if args.grow is not None:
        if not (args.tree or args.components_only):
            parser.error("--grow FILE grows a stored tree (--tree) or stored components (--components-only --edge-thresh SIM); give one of them")
        if args.components_only and args.edge_thresh is None:
            parser.error("--grow with --components-only needs the --edge-thresh SIM the stored components were filled at")
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--no-matrix", args.no_matrix), ("--nearest", args.nearest is not None),
                            ("--extend", args.extend is not None)):
            if given:
                parser.error(f"--grow goes with exactly one of --tree and --components-only; it cannot be combined with {flag}")
        if args.gpus > 1:
            parser.error("--grow: growing a stored result is a one-GPU call; it cannot be combined with --gpus N")
    if args.grow_nearest is not None:
        if args.nearest is None:
            parser.error("--grow-nearest FILE grows the stored lists of a --nearest K run; give --nearest K")
        if args.gpus > 1:
            parser.error("--grow-nearest: growing a stored result is a one-GPU call; it cannot be combined with --gpus N")
    if args.place is not None:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--no-matrix", args.no_matrix),
                            ("--nearest", args.nearest is not None), ("--tree", args.tree), ("--extend", args.extend is not None),
                            ("--grow", args.grow is not None), ("--cluster-table", args.cluster_table), ("--cluster-fit", args.cluster_fit)):
            if given:
                parser.error(f"--place stops after a placement of its own; it cannot be combined with {flag}")
        if args.gpus > 1:
            parser.error("--place: placing new genomes is a one-GPU call; it cannot be combined with --gpus N")
    if args.grow_table is not None and args.place is None:
        parser.error("--grow-table FILE grows the cluster table of the run that wrote the --place FIT file; give --place FIT")
    if args.join_min is not None:
        if args.grow_table is None:
            parser.error("--join-min SIM decides which new genomes join a cluster of --grow-table FILE; give --grow-table FILE")
        if not 0.0 <= args.join_min <= 1.0:              # (also refuses NaN)
            parser.error("--join-min is a similarity in [0, 1]")
    if args.cluster_table:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--tree", args.tree),
                            ("--nearest", args.nearest is not None), ("--extend", args.extend is not None)):
            if given:
                parser.error(f"--cluster-table reads the final clusters of the whole pipeline; it cannot be combined with {flag}")
    if args.cluster_fit:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--tree", args.tree),
                            ("--nearest", args.nearest is not None), ("--extend", args.extend is not None)):
            if given:
                parser.error(f"--cluster-fit reads the final clusters of the whole pipeline; it cannot be combined with {flag}")
    if args.no_matrix:
        for flag, given in (("--extend", args.extend is not None), ("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only)):
            if given:
                parser.error(f"--no-matrix runs the whole pipeline without the dense matrix; it cannot be combined with {flag}")
        if args.gpus > 1:
            parser.error("--no-matrix: the components and groups fills are one-GPU calls; it cannot be combined with --gpus N")
    if args.pairs is not None:
        for flag, given in (("--adjacency-only", args.adjacency_only), ("--components-only", args.components_only), ("--no-matrix", args.no_matrix),
                            ("--nearest", args.nearest is not None), ("--tree", args.tree), ("--distribution-only", args.distribution_only),
                            ("--distribution", args.distribution), ("--extend", args.extend is not None), ("--grow", args.grow is not None),
                            ("--place", args.place is not None), ("--cluster-table", args.cluster_table), ("--cluster-fit", args.cluster_fit),
                            ("--prefilter", args.prefilter)):
            if given:
                parser.error(f"--pairs stops after a pair-list fill of its own; it cannot be combined with {flag}")
        if args.gpus > 1:
            parser.error("--pairs: the pair-list fill is a one-GPU call; it cannot be combined with --gpus N")
    if args.prefilter:
        if not args.adjacency_only:
            parser.error("--prefilter bounds the edge list of --adjacency-only; give --adjacency-only -m peq --edge-thresh SIM")
        if args.metric != "peq":
            parser.error(f"--prefilter is the af bound of peq; it serves no other metric (-m {args.metric})")
        if args.edge_thresh is None:
            parser.error("--prefilter needs --edge-thresh SIM: without a threshold every pair that shares a pham is a candidate")
        if args.gpus > 1:
            parser.error("--prefilter: the pair-list fill is a one-GPU call; it cannot be combined with --gpus N")
    if args.also is not None:
        names = [name.strip() for name in args.also.split(",")]
        for name in names:
            if name not in METRICS:
                parser.error(f"--also names metrics among {', '.join(METRICS)}, separated by commas; '{name}' is none of them")
            if name == args.metric:
                parser.error(f"--also names metrics BESIDE -m's; '{name}' is -m's own")
            if names.count(name) > 1:
                parser.error(f"--also names every metric once; '{name}' is listed twice")
        for flag, given in (("--extend", args.extend is not None), ("--no-matrix", args.no_matrix), ("--adjacency-only", args.adjacency_only),
                            ("--components-only", args.components_only), ("--nearest", args.nearest is not None), ("--tree", args.tree),
                            ("--distribution-only", args.distribution_only), ("--place", args.place is not None), ("--grow", args.grow is not None),
                            ("--grow-nearest", args.grow_nearest is not None), ("--prefilter", args.prefilter), ("--af-bound", args.af_bound)):
            if given:
                parser.error(f"--also fills further metrics on the dense route or with --pairs; it cannot be combined with {flag}")
        if args.gpus > 1:
            parser.error("--also: the joint fill is a one-GPU call; it cannot be combined with --gpus N")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            parser.error("--also: the joint fill is a one-GPU call; it cannot be combined with a launcher job (WORLD_SIZE > 1)")
        args.also = names
    if args.af_bound:
        if args.nearest is None:
            parser.error("--af-bound bounds the alignments of --nearest K; give --nearest K -m peq")
        if args.metric != "peq":
            parser.error(f"--af-bound is the af bound of peq; it serves no other metric (-m {args.metric})")
        if args.grow_nearest is not None:
            parser.error("--af-bound fills the lists from scratch; it cannot be combined with --grow-nearest")
        if args.gpus > 1:
            parser.error("--af-bound: the pair-list fill is a one-GPU call; it cannot be combined with --gpus N")
    return args
