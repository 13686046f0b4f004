"""The pair distribution on the host (no GPU): the bindings of pc_fill_hist and its kin, ``PairDistribution.from_dense`` -- the host
statement of the definition -- against ``np.bincount`` and the dense matrix's own threshold counts on every dense golden file the
reference wrote, the exact statistics against an independent ``fractions`` computation and against the reference-style float
``SymMatrix.statistics``, the separation of a partition against a brute-force scan, the arithmetic of the class (sum, growth, files,
refusals), and the references of tests/hist_value_cases.py that the GPU cases are held to."""

import ctypes
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, REPO, golden_file, read_lower_triangle

NEW_EXPORTS = ("pc_fill_hist", "pc_multi_fill_hist", "pc_fill_rows_hist", "pc_last_hist_times", "pc_hist_bins", "pc_hist_table_slots", "pc_hist_probes")
MILLION = 10 ** 6
# |SymMatrix.statistics - exact| / |exact| on the six golden matrices (23 genomes, 253 pairs), measured on the CPU with this file's own
# fractions arithmetic: the reference-style property sums 253 floats left to right, the exact value is one correctly rounded
# conversion.  Largest per statistic over gcs, jc, pocp, af, aai, peq:
#   mean 1.53e-16 (af)   standard deviation 1.62e-15 (aai)   skewness 9.90e-15 (aai)
MEASURED_REL_DIFF = 9.90e-15
STATISTICS_BOUND = 10 * MEASURED_REL_DIFF


def dense_matrix(metric):
    from phamclust_amd.matrix import SymMatrix
    names, condensed, _ = read_lower_triangle(golden_file(metric))
    return SymMatrix.from_condensed(names, condensed, is_distance=True)


def micros(matrix):
    values = matrix.to_ndarray(condensed=True)
    k = np.rint(values * 1.0e6).astype(np.int64)
    assert np.array_equal(k / 1.0e6, values)
    return k


def pipeline_groups(names):
    """The clusters of the reference's own jc pipeline run on the golden input, every unclustered genome a group of its own."""
    fixture = json.load(open(os.path.join(GOLDEN, "pipeline_jc", "tree.json")))
    clusters = {}
    for rel in fixture["files"]:
        found = re.fullmatch(r"(cluster_\d+)/genomes/(.+)\.faa", rel)
        if found:
            clusters.setdefault(found.group(1), []).append(found.group(2))
    groups = [sorted(members) for _, members in sorted(clusters.items())]
    taken = {name for group in groups for name in group}
    assert len(groups) >= 2 and taken <= set(names)
    return groups + [[name] for name in names if name not in taken]


# ---- binding ----------------------------------------------------------------------------------------------------------
def test_hist_is_exported_everywhere(native_built):
    from phamclust_amd import hip, matrix
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    for name in ("pc_fill_hist", "pc_multi_fill_hist", "pc_fill_rows_hist"):
        assert name in design and name in integration, name
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 170 and hip.load().pc_version() >= 170
    assert hip.load().pc_hist_bins() == hip.HIST_BINS == matrix.HIST_BINS == MILLION + 1
    slots = hip.Context.hist_table_slots()
    assert slots & (slots - 1) == 0 and 2 * slots * 8 <= 160 * 1024 // 2, "two or more workgroups' tables fit a CU's LDS"
    assert 1 <= hip.Context.hist_probes() < slots
    assert hip.Context.hist_slot(0) == 0 and 0 <= hip.Context.hist_slot((1 << 20) | MILLION) < slots
    for owner in (hip.Context, hip.MultiContext):
        assert hasattr(owner, "fill_hist")
    assert hasattr(hip.Context, "fill_rows_hist") and len(hip.load().pc_fill_rows_hist.argtypes) == 14
    for name in ("PairDistribution", "distribution_de_novo", "distribution_extend", "distribution_to_file", "distribution_from_file"):
        assert hasattr(matrix, name), name
    # the value hooks' comments list the new walks
    assert re.search(r"_between, _affinity, _hist and their pc_multi_ forms", header) and re.search(r"_affinity, _between, _hist\.  The rows fill", header)


@pytest.mark.parametrize("symbol", ["pc_fill_hist", "pc_multi_fill_hist", "pc_fill_rows_hist"])
def test_library_refuses_before_upload(native_built, symbol):
    """No context: a refusal, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    junk = (ctypes.c_int64 * 1)(1)
    ph = ctypes.cast(junk, ctypes.POINTER(ctypes.c_int64))
    ncl, npairs, nsl = ctypes.c_int32(5), ctypes.c_int64(5), ctypes.c_int32(5)
    outs = (ctypes.byref(ph), ctypes.byref(ncl), ctypes.byref(npairs), ctypes.byref(nsl), None)
    if symbol == "pc_fill_rows_hist":
        rows = (ctypes.c_int32 * 1)(0)
        rc = lib.pc_fill_rows_hist(None, 1, 1, None, 0, rows, 1, None, 0, *outs)
    else:
        rc = getattr(lib, symbol)(None, 1, 1, None, 0, 0, *outs)
    assert rc != 0 and symbol.encode() in lib.pc_last_error()
    assert not ph and ncl.value == 0 and npairs.value == 0 and nsl.value == 0


# ---- the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_from_dense_is_the_bincount_and_the_threshold_counts(metric):
    from phamclust_amd.matrix import PairDistribution, SparseEdges
    matrix = dense_matrix(metric)
    k = micros(matrix)
    dist = PairDistribution.from_dense(matrix)
    dense = np.bincount(k, minlength=MILLION + 1)
    assert np.array_equal(dist.to_hist(), dense[None, :]) and dist.n_pairs == k.shape[0] == len(matrix) * (len(matrix) - 1) // 2
    assert np.array_equal(dist.micro, np.flatnonzero(dense)) and np.array_equal(dist.count, dense[np.flatnonzero(dense)])
    assert dist.is_distance and dist.nodes == matrix.nodes and not dist.partitioned
    assert dist.min == k.min() / 1.0e6 and dist.max == k.max() / 1.0e6
    values = matrix.to_ndarray(condensed=True)
    for threshold in sorted({0.0, 1.0, 0.5, 0.25, float(np.median(values)), float(values.min()), float(values.max()), 0.999999}):
        for strict in (False, True):
            want = int((values < threshold).sum() if strict else (values <= threshold).sum())
            assert dist.count_within(threshold, strict) == want, (threshold, strict)
        # the dense matrix's own statement: the neighbours within a threshold, every pair from both ends
        assert 2 * dist.count_within(threshold) == sum(len(matrix.nearest_neighbors(name, threshold)) for name in matrix.nodes), threshold
        assert dist.count_within(threshold) == len(SparseEdges.from_dense(matrix, threshold)), threshold
    # the similarity direction: the inverted matrix's histogram, every millionth's complement
    inverted = dense_matrix(metric)
    inverted.invert()
    sim = PairDistribution.from_dense(inverted)
    assert sim == dist.inverted() and not sim.is_distance and sim.inverted() == dist
    for threshold in (0.0, 0.35, 0.75, 1.0):
        assert sim.count_within(threshold) == int((1.0e6 - k >= np.rint(threshold * 1.0e6)).sum())
        assert 2 * sim.count_within(threshold) == sum(len(inverted.nearest_neighbors(name, threshold)) for name in inverted.nodes)
    # quantiles: the smallest value with at least ceil(q n) pairs at or below it
    ordered = np.sort(k)
    for q in (0, Fraction(1, 4), Fraction(1, 2), Fraction(3, 4), Fraction(1, 3), 1, 0.9):
        rank = max(1, math.ceil(Fraction(q) * ordered.shape[0]))
        assert dist.quantile(q) == ordered[rank - 1] / 1.0e6, q
    assert dist.median == dist.quantile(0.5)
    value, pairs = dist.cumulative()
    assert np.array_equal(pairs, [dist.count_within(v) for v in value]) and pairs[-1] == dist.n_pairs
    sim_value, sim_pairs = sim.cumulative()
    assert np.array_equal(sim_pairs, [sim.count_within(v) for v in sim_value]) and sim_pairs[0] == sim.n_pairs
    for budget in (0, 1, 10, 100, dist.n_pairs - 1, dist.n_pairs, dist.n_pairs + 5):
        for d in (dist, sim):
            t = d.threshold_for(budget)
            if t is None:
                assert d.count_within(0.0 if d.is_distance else 1.0) > budget
                continue
            assert d.count_within(t) <= budget
            looser = round(t + (1e-6 if d.is_distance else -1e-6), 6)
            assert not 0.0 <= looser <= 1.0 or d.count_within(looser) > budget, (budget, t)


def exact_statistics(k):
    """mean, sample standard deviation and sample skewness (the reference's forms) of the millionths k, each ONE correctly rounded
    conversion of an exact rational (the deviation and the skewness: of their exact squares, then the square root)."""
    values = [Fraction(int(x), MILLION) for x in k]
    n = len(values)
    mean = sum(values) / n
    q2 = sum((v - mean) ** 2 for v in values)
    q3 = sum((v - mean) ** 3 for v in values)
    var = q2 / (n - 1)
    if q2 == 0:
        return float(mean), 0.0, 0.0
    skew_sq = q3 * q3 / ((n - 1) ** 2 * var ** 3)
    return float(mean), math.sqrt(float(var)), math.copysign(math.sqrt(float(skew_sq)), q3) if q3 else 0.0


@pytest.mark.parametrize("metric", ALL_METRICS)
def test_statistics_are_exact(metric):
    from phamclust_amd.matrix import PairDistribution
    matrix = dense_matrix(metric)
    dist = PairDistribution.from_dense(matrix)
    want = exact_statistics(micros(matrix))
    assert dist.statistics == want                                           # to the last bit
    assert (dist.mean, dist.std_dev(), dist.skewness()) == want
    n = dist.n_pairs
    assert dist.std_dev(sample=False) == math.sqrt(float(dist.variance_exact() * (n - 1) / n))
    # the reference-style float property sums in another order: within ten times the largest difference measured for it (above)
    got = matrix.statistics
    for a, b, what in zip(got, want, ("mean", "std", "skew")):
        rel = abs(a - b) / abs(b)
        print(f"{metric} {what}: SymMatrix.statistics {a!r}, exact {b!r}, relative difference {rel:.3e}")
        assert rel <= STATISTICS_BOUND, (what, a, b)


def test_statistics_conventions():
    from phamclust_amd.matrix import PairDistribution
    flat = PairDistribution(([250000], [7]))
    assert flat.statistics == (0.25, 0.0, 0.0) and flat.min == flat.max == flat.median == 0.25
    single = PairDistribution(([999999], [1]))
    assert single.statistics == (0.999999, 0.0, 0.0)
    with pytest.raises(ValueError, match="no pairs"):
        PairDistribution(([], [])).mean
    big = PairDistribution(([0, MILLION], [2 ** 40, 2 ** 40]))                # sums far beyond 2^64: Python integers
    assert big.mean == 0.5 and big.skewness() == 0.0 and abs(big.std_dev() - 0.5) < 1e-12


# ---- a partition ----------------------------------------------------------------------------------------------------------
def test_separation_against_a_brute_force_scan():
    from phamclust_amd.matrix import PairDistribution
    matrix = dense_matrix("jc")
    names = matrix.nodes
    groups = pipeline_groups(names)
    of = {name: a for a, group in enumerate(groups) for name in group}
    s, t = np.triu_indices(len(names), k=1)
    same = np.array([of[names[a]] == of[names[b]] for a, b in zip(s, t)])
    k = np.rint(np.asarray(matrix._ordered())[s, t] * 1.0e6).astype(np.int64)
    for source, values, is_distance in ((matrix, k, True), (None, MILLION - k, False)):
        if source is None:
            source = dense_matrix("jc")
            source.invert()
        dist = PairDistribution.from_dense(source, groups)
        assert dist.partitioned and dist.n_pairs == k.shape[0]
        assert dist.within.n_pairs == int(same.sum()) == sum(len(g) * (len(g) - 1) // 2 for g in groups)
        assert np.array_equal(dist.to_hist(), np.stack([np.bincount(values[same], minlength=MILLION + 1), np.bincount(values[~same], minlength=MILLION + 1)]))
        assert dist.whole == PairDistribution.from_dense(source) and dist.within + dist.between == dist.whole
        # every millionth as a threshold, by counting over the sorted raw values (no histogram)
        w_sorted, b_sorted = np.sort(values[same]), np.sort(values[~same])
        c = np.arange(MILLION + 1)
        if is_distance:
            beyond = w_sorted.shape[0] - np.searchsorted(w_sorted, c, side="right")
            inside = np.searchsorted(b_sorted, c, side="right")
        else:
            beyond = np.searchsorted(w_sorted, c, side="left")
            inside = b_sorted.shape[0] - np.searchsorted(b_sorted, c, side="left")
        for at in sorted({0, MILLION, 500000} | set(values.tolist())):
            passing = values <= at if is_distance else values >= at
            assert (int(beyond[at]), int(inside[at])) == (int((same & ~passing).sum()), int((~same & passing).sum()))
            assert dist.separation(at / 1.0e6) == (int(beyond[at]), int(inside[at])), at
        smallest = int(np.argmin(beyond + inside))                           # (the first minimum: the smallest threshold on ties)
        assert dist.best_separation() == (smallest / 1.0e6, int(beyond[smallest]), int(inside[smallest]))
    with pytest.raises(ValueError, match="not split"):
        PairDistribution.from_dense(matrix).separation(0.5)


# ---- arithmetic, growth, files ------------------------------------------------------------------------------------------------
def test_add_extended_and_the_file_round_trip(tmp_path):
    from phamclust_amd.matrix import PairDistribution, distribution_from_file, distribution_to_file
    matrix = dense_matrix("pocp")
    names = matrix.nodes
    n = len(names)
    groups = pipeline_groups(names)
    label = np.zeros(n, dtype=np.int64)
    for a, group in enumerate(groups):
        label[[names.index(x) for x in group]] = a
    square = np.asarray(matrix._ordered())
    for rows in ([n - 1], [0], [3, 4], [1, 7, 8, 20], list(range(n))):
        old = [g for g in range(n) if g not in rows]
        stored_matrix = matrix.extract_submatrix([names[g] for g in old])
        poisoned = square[rows].copy()
        poisoned[np.arange(len(rows)), rows] = np.nan                          # the diagonal is no pair: never looked at
        for part in (None, groups):
            whole = PairDistribution.from_dense(matrix, part)
            stored = PairDistribution.from_dense(stored_matrix, None if part is None else [[x for x in g if x in set(stored_matrix.nodes)] for g in part
                                                                                           if set(g) & set(stored_matrix.nodes)]) \
                if len(old) > 0 else PairDistribution([([], [])] * (1 if part is None else 2))
            grown = stored.extended(n, rows, poisoned, labels=None if part is None else label, nodes=names)
            assert grown == whole and grown.nodes == names
            stored.check_seed(len(old), None if part is None else label[old])
    whole = PairDistribution.from_dense(matrix, groups)
    with pytest.raises(ValueError, match="another genome set"):
        whole.check_seed(n - 1, label[:-1])
    with pytest.raises(ValueError, match="another partition"):
        whole.check_seed(n, np.zeros(n, dtype=np.int64))
    with pytest.raises(ValueError, match="needs the genomes' labels"):
        whole.extended(n, [0], square[[0]])
    with pytest.raises(ValueError, match="differ in direction or in their classes"):
        whole + whole.whole
    with pytest.raises(ValueError, match="differ in direction"):
        whole + whole.inverted()
    assert (whole + whole).n_pairs == 2 * whole.n_pairs and (whole + whole).mean == whole.mean
    # the files: non-empty bins, byte for byte through a round trip, in either direction and either form
    for k, dist in enumerate((whole, whole.whole, whole.inverted(), whole.whole.inverted())):
        path = distribution_to_file(dist, str(tmp_path / f"d{k}.tsv"))
        text = open(path).read()
        lines = text.splitlines()
        assert lines[0] == ("value\twithin\tbetween" if dist.partitioned else "value\tcount") and len(lines) == 1 + dist.micro.shape[0]
        assert all(re.fullmatch(r"[01]\.\d{6}(\t\d+)+", line) for line in lines[1:])
        back = distribution_from_file(path, is_distance=dist.is_distance, nodes=names)
        assert back == dist and back.nodes == names
        assert open(distribution_to_file(back, str(tmp_path / f"e{k}.tsv"))).read() == text
    bad = tmp_path / "bad.tsv"
    bad.write_text("value\tcount\n0.500000\t3\n0.400000\t1\n")
    with pytest.raises(ValueError, match="ascend"):
        distribution_from_file(str(bad))
    bad.write_text("source\ttarget\n")
    with pytest.raises(ValueError, match="no distribution file"):
        distribution_from_file(str(bad))


def test_constructor_refusals():
    from phamclust_amd.matrix import PairDistribution
    for bins, needle in (((([1, 0]), [1, 1]), "strictly ascending"), (([0, MILLION + 1], [1, 1]), "outside"), (([5], [-1]), "negative count"),
                         (([5, 6], [1]), "bins and")):
        with pytest.raises(ValueError, match=needle):
            PairDistribution(bins)
    with pytest.raises(ValueError, match="classes"):
        PairDistribution([([1], [1])] * 3)
    with pytest.raises(ValueError, match="from_hist"):
        PairDistribution.from_hist(np.zeros((1, 10), dtype=np.int64))
    kept = PairDistribution(([1, 2, 3], [4, 0, 5]))
    assert kept.micro.tolist() == [1, 3] and kept.count.tolist() == [4, 5]     # an empty bin is not kept


def test_extend_refusals_come_before_any_gpu_call(small_genomes):
    from phamclust_amd.cli import METRICS
    from phamclust_amd.matrix import PairDistribution, distribution_extend
    func = METRICS["jc"]
    names = [g.name for g in small_genomes]
    n_old = len(names) - 2
    good = PairDistribution(([MILLION], [n_old * (n_old - 1) // 2]), nodes=names[:n_old])
    with pytest.raises(ValueError, match="does not know its genomes"):
        distribution_extend(PairDistribution(([0], [1])), small_genomes, func)
    with pytest.raises(ValueError, match="groups is needed exactly when"):
        distribution_extend(good, small_genomes, func, groups=[names])
    with pytest.raises(ValueError, match="another genome set"):
        distribution_extend(PairDistribution(([MILLION], [5]), nodes=names[:n_old]), small_genomes, func)
    with pytest.raises(KeyError, match="not among the genomes"):
        distribution_extend(PairDistribution(([MILLION], [1]), nodes=["stranger", names[0]]), small_genomes, func)
    split = PairDistribution([([MILLION], [1]), ([MILLION], [n_old * (n_old - 1) // 2 - 1])], nodes=names[:n_old])
    with pytest.raises(ValueError, match="another partition"):
        distribution_extend(split, small_genomes, func, groups=[[x] for x in names])
    # nothing new: the stored distribution re-laid, no GPU call
    full = PairDistribution(([MILLION], [len(names) * (len(names) - 1) // 2]), nodes=names)
    assert distribution_extend(full, small_genomes, func) == full


# ---- the references of the GPU cases ------------------------------------------------------------------------------------------
def test_the_gpu_cases_references_are_from_dense():
    import hist_value_cases as cases
    import rows_value_cases as rowcases
    import slab_value_cases as tri
    from phamclust_amd.matrix import PairDistribution, SymMatrix
    n = 40
    names = [f"g{k:02d}" for k in range(n)]
    for values in (tri.spread(n, 5), tri.tie_set(n, 6), cases.all_distinct(n), cases.rotation(n, [0, MILLION]), cases.collide(n, 2048, 8, 7)):
        matrix = SymMatrix.from_condensed(names, tri.square(values, n)[np.triu_indices(n, k=1)], is_distance=True)
        for label, (group, n_groups) in cases.labelings(n).items():
            groups = [[names[g] for g in np.flatnonzero(group == a)] for a in range(n_groups)]
            groups = [g for g in groups if g]
            dist = PairDistribution.from_dense(matrix, groups)
            assert np.array_equal(dist.to_hist(), cases.hist(values, n, group)), label
            assert np.array_equal(dist.inverted().to_hist(), cases.hist(values, n, group, as_distance=False)), label
            assert int(cases.hist(values, n, group)[0].sum()) == cases.within_pairs(group)
        assert np.array_equal(PairDistribution.from_dense(matrix).to_hist(), cases.hist(values, n))
        rows = rowcases.as_rows([2, 3, 19, 39])
        old = ~rowcases.query_mask(rows, n)
        sub = matrix.extract_submatrix([names[g] for g in np.flatnonzero(old)])
        assert np.array_equal(PairDistribution.from_dense(sub).to_hist(), cases.hist_among(values, n, old))
        slab = rowcases.poisoned(rowcases.rows_of(values, n, rows), rows, n, float("nan"), 7.0)
        grown = PairDistribution.from_dense(sub).extended(n, rows, slab)
        assert np.array_equal(grown.to_hist(), cases.hist(values, n))
    slots = 2048
    run = cases.colliding_micros(slots, 20)
    assert len({cases.slot_of(int(m), slots) for m in run}) == 1 and np.unique(run).shape[0] == 20
    bad = cases.with_bad(tri.spread(n, 8), [0, 1, 2, 3, 4])
    k = np.rint(bad[:5] * 1.0e6)
    assert all(not (0 <= x <= MILLION) or x / 1.0e6 != v for x, v in zip(k, bad[:5]))      # none of them is a millionth in [0, 1]


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_distribution_command_line(capsys):
    import inspect
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--distribution-only", "-e", "0.3", "--gpus", "2"])
    assert args.distribution_only and not args.distribution and args.edge_thresh == 0.3 and args.gpus == 2
    assert cli.parse_args(["in.tsv", "out", "-H"]).distribution_only and cli.parse_args(["in.tsv", "out", "-U", "--no-matrix"]).distribution
    assert cli.DEFAULTS["distribution_only"] is False and cli.DEFAULTS["distribution"] is False
    assert cli.parse_args(["in.tsv", "out", "--distribution", "--cluster-table", "--cluster-fit"]).distribution
    for bad in (["--adjacency-only"], ["--components-only"], ["--no-matrix"], ["--nearest", "3"], ["--tree"], ["--extend", "old.tsv"],
                ["--place", "fit.tsv"], ["--cluster-table"], ["--cluster-fit"], ["--distribution"], ["--tree", "--grow", "f"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--distribution-only"] + bad)
        assert "--distribution-only" in capsys.readouterr().err or bad == ["--tree", "--grow", "f"], bad
    for bad in (["--adjacency-only"], ["--components-only"], ["--nearest", "3"], ["--tree"], ["--extend", "old.tsv"], ["--place", "fit.tsv"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--distribution"] + bad)
    help_text = cli.build_parser().format_help()
    assert "--distribution-only" in help_text and "--distribution " in help_text.replace("\n", " ")
    # several GPUs: from one process; under the launcher route the stage stays on one GPU and says why
    plan = script.gpus_plan(cli.parse_args(["in.tsv", "out", "--distribution-only", "--gpus", "2"]), "launcher", None)
    assert plan[:2] == (1, "one") and "--distribution-only" in plan[2]
    assert script.gpus_plan(cli.parse_args(["in.tsv", "out", "--distribution-only", "--gpus", "2"]), "process", None)[:2] == (2, "process")
    # the pipeline function refuses the same combinations before a file is read or a GPU touched
    params = inspect.signature(script.phamclust).parameters
    assert params["distribution_only"].default is False and params["distribution"].default is False
    base = (None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    for bad in (dict(distribution_only=True, tree=True), dict(distribution_only=True, distribution=True), dict(distribution_only=True, no_matrix=True),
                dict(distribution_only=True, nearest=3), dict(distribution_only=True, extend="old.tsv"), dict(distribution=True, adjacency_only=True),
                dict(distribution=True, place="fit.tsv"), dict(distribution=True, extend="old.tsv"), dict(distribution=True, edge_thresh=0.3)):
        with pytest.raises(ValueError):
            script.phamclust(*base, **bad)
