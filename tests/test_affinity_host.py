"""The affinity fill on the host (no GPU): the binding of pc_fill_affinity, ``GroupAffinity.from_dense`` -- the host statement of the
definition -- against brute force over ``SymMatrix.get_weight`` on every dense golden file, what the class derives from it (medoids,
silhouettes, the folded between-groups table, the inverted statement, the file), the host arithmetic of the table's size, and the
refusals that come before any GPU call.  Every comparison is exact (integers, ``np.array_equal``) but the silhouette against
scikit-learn's, whose bound is derived where it is asserted."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ALL_METRICS, REPO
from test_between_host import EMPTY, dense_matrix, partitions

NEW_EXPORTS = ("pc_fill_affinity", "pc_multi_fill_affinity", "pc_last_affinity_times", "pc_affinity_block", "pc_affinity_bytes")
EMPTY_ENTRY = EMPTY[1:]                              # sum, lo, hi of an entry no pair falls into
MILLION = 1000000


# ---- binding ------------------------------------------------------------------------------------------------------
def test_affinity_is_exported_everywhere(native_built):
    from phamclust_amd import hip, matrix
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b(int|int64_t) " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 165 and hip.load().pc_version() >= 165
    assert hip.Context.affinity_block() == hip.load().pc_affinity_block() >= 1
    assert hasattr(hip.Context, "fill_affinity") and hasattr(hip.MultiContext, "fill_affinity")
    assert hasattr(matrix, "GroupAffinity") and hasattr(matrix, "affinity_de_novo")


def test_affinity_bytes_arithmetic(native_built):
    """16 bytes per entry and the 8-byte violation count; what cannot be represented is refused, not wrapped."""
    from phamclust_amd import hip
    lib = hip.load()
    for n, g in ((0, 1), (1, 1), (200, 7), (20000, 800), (20000, 2048), (1 << 22, 2048)):
        assert hip.Context.affinity_bytes(n, g) == lib.pc_affinity_bytes(n, g) == 16 * n * g + 8, (n, g)
    assert hip.Context.affinity_bytes(20000, 800) == 256000008 and hip.Context.affinity_bytes(20000, 2048) == 655360008
    assert lib.pc_affinity_bytes(-1, 4) == -1 and lib.pc_affinity_bytes(4, -1) == -1
    assert lib.pc_affinity_bytes(1 << 40, 1 << 40) == -1                   # above 2^63
    with pytest.raises(ValueError):
        hip.Context.affinity_bytes(1 << 40, 1 << 40)


@pytest.mark.parametrize("symbol", ["pc_fill_affinity", "pc_multi_fill_affinity"])
def test_library_refuses_before_upload(native_built, symbol):
    """No context: a refusal, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    junk_i, junk_l = (ctypes.c_int32 * 1)(1), (ctypes.c_int64 * 1)(1)
    kinds = (i64p, i32p, i32p, i32p, i64p, i32p, i32p, i64p, i32p, i32p)
    cells = [ctypes.cast(junk_l if kind is i64p else junk_i, kind) for kind in kinds]
    nsl = ctypes.c_int32(5)
    group = (ctypes.c_int32 * 1)(0)
    rc = getattr(lib, symbol)(None, 1, 1, group, 1, 1, 0, *(ctypes.byref(cell) for cell in cells), ctypes.byref(nsl), None)
    assert rc != 0 and symbol.encode() in lib.pc_last_error()
    assert not any(bool(cell) for cell in cells) and nsl.value == 0
    assert lib.pc_last_affinity_times(None, None, None, None) != 0


# ---- the definition against brute force ------------------------------------------------------------------------------
def brute_table(matrix, groups):
    """{(genome index, group): the millionths of every pair of the genome with a member of the group}, by Python loops."""
    names = matrix.nodes
    lists = {}
    for i, first in enumerate(names):
        for b, group in enumerate(groups):
            for second in group:
                if second == first:
                    continue
                w = matrix.get_weight(first, second)
                k = int(round(w * MILLION))
                assert k / MILLION == w
                lists.setdefault((i, b), []).append(k)
    return lists


def brute_nearest(lists, groups, label, i):
    """The other non-empty group nearest to genome i by each criterion on DISTANCE lists, ties to the smaller index, in Python integers."""
    best = [None, None, None]
    for b, group in enumerate(groups):
        if b == label[i] or not group:
            continue
        ks = lists[(i, b)]
        keys = (None, min(ks), max(ks))
        for c in (1, 2):
            if best[c] is None or keys[c] < best[c][0]:
                best[c] = (keys[c], b)
        if best[0] is None or sum(ks) * best[0][1] < best[0][0] * len(ks):
            best[0] = (sum(ks), len(ks), b)
    return best


def check_against_brute(found, matrix, groups, tag):
    names = matrix.nodes
    label = {i: b for b, group in enumerate(groups) for i in [names.index(x) for x in group]}
    lists = brute_table(matrix, groups)
    dist = lists if matrix.is_distance else {key: [MILLION - k for k in ks] for key, ks in lists.items()}
    total, lo, hi = found.table
    counts = found.counts()
    for i in range(len(names)):
        for b in range(len(groups)):
            ks = lists.get((i, b))
            want = (sum(ks), min(ks), max(ks)) if ks else EMPTY_ENTRY
            assert (int(total[i, b]), int(lo[i, b]), int(hi[i, b])) == want, (tag, i, b)
            assert counts[i, b] == (len(ks) if ks else 0), (tag, i, b)
        own = lists.get((i, label[i]))
        want = (sum(own), min(own), max(own)) if own else EMPTY_ENTRY
        assert (int(found.own_sum[i]), int(found.own_lo[i]), int(found.own_hi[i])) == want, (tag, i)
        best = brute_nearest(dist, groups, label, i)
        if best[0] is None:
            assert found.near_group[:, i].tolist() == [-1, -1, -1], (tag, i)
            assert (int(found.near_sum[i]), int(found.near_lo[i]), int(found.near_hi[i])) == EMPTY_ENTRY, (tag, i)
            continue
        assert found.near_group[:, i].tolist() == [best[0][2], best[1][1], best[2][1]], (tag, i)
        flip = (lambda k, n=1: k) if matrix.is_distance else (lambda k, n=1: n * MILLION - k)
        assert int(found.near_sum[i]) == flip(best[0][0], best[0][1]), (tag, i)
        assert (int(found.near_lo[i]), int(found.near_hi[i])) == (flip(best[1][0]), flip(best[2][0])), (tag, i)


@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_from_dense_and_what_follows_from_it(tmp_path, name, metric):
    from sklearn.metrics import silhouette_samples
    from phamclust_amd.matrix import GroupAffinity, GroupLinkage, affinity_from_file, affinity_to_file
    matrix = dense_matrix(name, metric)
    similar = matrix.extract_submatrix(matrix.nodes).invert()
    square = matrix.to_ndarray()
    names = matrix.nodes
    for tag, groups in partitions(matrix).items():
        label = (name, metric, tag)
        found = GroupAffinity.from_dense(matrix, groups)
        assert found.is_distance and found.nodes == names and found.own_sum.dtype == found.near_sum.dtype == np.int64, label
        assert found.own_lo.dtype == found.near_group.dtype == found.table[1].dtype == np.int32 and found.near_group.shape == (3, len(names)), label
        check_against_brute(found, matrix, groups, label)
        # the inverted statement is the inverted matrix's
        inverted = found.inverted()
        assert not inverted.is_distance and inverted == GroupAffinity.from_dense(similar, groups) and inverted.inverted() == found, label
        check_against_brute(inverted, similar, groups, label)
        assert np.array_equal(inverted.near_group, found.near_group), label
        # the rows of a group folded give the between-groups table
        assert found.folded() == GroupLinkage.from_dense(matrix, groups) and inverted.folded() == GroupLinkage.from_dense(similar, groups), label
        with pytest.raises(ValueError):
            GroupAffinity.from_dense(matrix, groups, want_table=False).folded()
        # medoids: SymMatrix.medoid of every group's own sub-matrix
        medoids = found.medoids()
        for a, group in enumerate(groups):
            assert medoids[a] == matrix.extract_submatrix(group).medoid[0], (label, a)
        # silhouettes.  Both sides add at most N = 200 values in [0, 1] in fp64: each mean is off by at most N * 2^-53 relative, the
        # quotient by a few times that -- orders of magnitude below the 5e-9 a one-millionth error in one value would cause.
        sizes = [len(group) for group in groups]
        silhouette = found.silhouette()
        assert np.array_equal(silhouette, inverted.silhouette(), equal_nan=True), label
        if sum(1 for s in sizes if s) >= 2:
            of = {x: a for a, group in enumerate(groups) for x in group}
            if len(groups) < len(names):
                want = silhouette_samples(square, np.array([of[x] for x in names]), metric="precomputed")
            else:                                                           # (scikit-learn refuses as many labels as samples; by its
                want = np.zeros(len(names))                                 # convention every genome alone in its group scores 0)
            assert np.abs(silhouette - want).max() <= 1e-12, (label, float(np.abs(silhouette - want).max()))
            at = {x: k for k, x in enumerate(names)}
            by_group = found.silhouette_by_group()
            for a, group in enumerate(groups):
                assert by_group[a] == float(np.mean(silhouette[[at[x] for x in group]])), (label, a)
                if len(group) == 1:
                    assert silhouette[at[group[0]]] == 0.0, (label, a)
            assert found.silhouette_mean() == float(np.mean(silhouette)), label
        else:
            assert np.isnan(silhouette).all() and np.isnan(found.silhouette_mean()), label
        # what a caller reads per genome
        for kind, row, values in (("mean", 0, None), ("nearest", 1, found.near_lo), ("farthest", 2, found.near_hi)):
            assert np.array_equal(found.nearest_group(kind), found.near_group[row]), label
            value = found.nearest_value(kind)
            there = found.near_group[row] >= 0
            assert np.isnan(value[~there]).all(), label
            if values is not None:
                assert np.array_equal(value[there], values[there] / 1.0e6), label
            else:
                assert np.array_equal(value[there], found.near_sum[there] / (found.sizes[found.near_group[0][there]] * 1.0e6)), label
        first = groups[0][0]
        assert (np.isnan(found.own_mean(first)) if sizes[0] == 1 else
                found.own_mean(first) == int(found.own_sum[names.index(first)]) / ((sizes[0] - 1) * MILLION)), label
        with pytest.raises(ValueError):
            found.nearest_group("median")
        # the file
        for one in (found, inverted):
            plain = GroupAffinity.from_dense(matrix if one.is_distance else similar, groups, want_table=False)
            path = affinity_to_file(one, tmp_path / "affinity.tsv")
            back = affinity_from_file(path)
            assert back == plain and back.table is None and back != one, label
            assert len(open(path).read().splitlines()) == 2 + len(names), label


def test_empty_groups_single_group_and_given_order():
    from phamclust_amd.matrix import GroupAffinity, SymMatrix, affinity_from_file
    names = ["a", "b", "c", "d"]
    matrix = SymMatrix.from_condensed(names, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], is_distance=True)      # ab ac ad bc bd cd
    found = GroupAffinity.from_dense(matrix, [["c", "a"], [], ["d"], ["b"]])                       # group 1 is empty
    total, lo, hi = found.table
    assert total.tolist() == [[200000, 0, 300000, 100000], [500000, 0, 500000, 0], [200000, 0, 600000, 400000], [900000, 0, 0, 500000]]
    assert lo[:, 1].tolist() == [EMPTY_ENTRY[1]] * 4 and hi[:, 1].tolist() == [-1] * 4
    assert (int(total[3, 2]), int(lo[3, 2]), int(hi[3, 2])) == EMPTY_ENTRY and (int(lo[0, 0]), int(hi[0, 0])) == (200000, 200000)
    assert found.counts().tolist() == [[1, 0, 1, 1], [2, 0, 1, 0], [1, 0, 1, 1], [2, 0, 0, 1]]
    assert found.own_sum.tolist() == [200000, 0, 200000, 0] and found.own_lo.tolist() == [200000, EMPTY_ENTRY[1], 200000, EMPTY_ENTRY[1]]
    assert found.near_group.tolist() == [[3, 0, 3, 0], [3, 0, 3, 0], [3, 0, 3, 3]]         # (the empty group is never nearest)
    assert found.near_sum.tolist() == [100000, 500000, 400000, 900000]
    assert found.medoids() == ["c", None, "d", "b"]                                        # a tie: the first member in the given order
    assert GroupAffinity.from_dense(matrix, [["a", "c"], [], ["d"], ["b"]]).medoids()[0] == "a"
    assert np.isnan(found.silhouette_by_group()[1])
    assert found.silhouette().tolist() == [(0.1 - 0.2) / 0.2, 0.0, (0.4 - 0.2) / 0.4, 0.0]
    one = GroupAffinity.from_dense(matrix, [names])
    assert one.near_group.tolist() == [[-1] * 4] * 3 and one.near_lo.tolist() == [EMPTY_ENTRY[1]] * 4 and one.near_hi.tolist() == [-1] * 4
    assert np.isnan(one.silhouette()).all() and np.isnan(one.nearest_value("mean")).all()
    assert one.own_sum.tolist() == [600000, 1000000, 1200000, 1400000] and one.medoids() == ["a"]
    assert one.inverted().medoids() == ["a"] and one.inverted().own_sum.tolist() == [2400000, 2000000, 1800000, 1600000]
    for groups in ([["a"], ["a", "b", "c", "d"]], [["a", "b", "c"]], [["a", "b", "c", "x"], ["d"]]):
        with pytest.raises((ValueError, KeyError)):
            GroupAffinity.from_dense(matrix, groups)
    with pytest.raises(ValueError):
        GroupAffinity(names, [names], [0] * 3, [0] * 4, [0] * 4, np.zeros((3, 4)), [0] * 4, [0] * 4, [0] * 4)
    with pytest.raises(ValueError):
        affinity_from_file(os.path.join(REPO, "README.md"))


# ---- refusals, before any GPU call ------------------------------------------------------------------------------------
def test_fill_affinity_refuses_its_arguments_before_the_library():
    from phamclust_amd import hip

    class Packed:
        n_genomes = 4

    ctx = object.__new__(hip.Context)
    ctx._packed, ctx._h, ctx._lib = Packed(), None, None                    # (any library call would fail on None)
    with pytest.raises(ValueError, match="group is None"):
        ctx.fill_affinity("jc", None)
    with pytest.raises(ValueError, match="3 labels for 4 genomes"):
        ctx.fill_affinity("jc", [0, 1, 2])


def test_affinity_de_novo_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import matrix
    from phamclust_amd.cli import METRICS

    def no_gpu(*args, **kwargs):
        raise AssertionError("a GPU call was reached")
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_multi_context", no_gpu)
    names = [g.name for g in small_genomes]
    with pytest.raises(ValueError, match="METRICS"):
        matrix.affinity_de_novo(small_genomes, lambda a, b: 0.5, [names])
    with pytest.raises(ValueError, match="is in no group"):
        matrix.affinity_de_novo(small_genomes, METRICS["jc"], [names[1:]])
    with pytest.raises(ValueError, match="is in groups 0 and 1"):
        matrix.affinity_de_novo(small_genomes, METRICS["jc"], [names, names[:1]])
    with pytest.raises(KeyError):
        matrix.affinity_de_novo(small_genomes, METRICS["jc"], [names, ["nobody"]])
    with pytest.raises(ValueError, match="groups"):
        matrix.affinity_de_novo(small_genomes, METRICS["jc"], [names] + [[] for _ in range(matrix.BETWEEN_MAX_GROUPS)])
    with pytest.raises(ValueError, match="groups"):
        matrix.affinity_de_novo(small_genomes, METRICS["jc"], [])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="launcher"):
        matrix.affinity_de_novo(small_genomes, METRICS["jc"], [names])


def test_cluster_fit_command_line(capsys):
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "--cluster-fit", "--no-matrix"])
    assert args.cluster_fit and args.no_matrix and cli.DEFAULTS["cluster_fit"] is False
    assert cli.parse_args(["in.tsv", "out", "--cluster-fit", "--gpus", "2"]).gpus == 2
    both = cli.parse_args(["in.tsv", "out", "--cluster-fit", "--cluster-table"])
    assert both.cluster_fit and both.cluster_table
    assert not cli.parse_args(["in.tsv", "out"]).cluster_fit
    for other in (["--adjacency-only"], ["--components-only"], ["--tree"], ["--nearest", "3"], ["--extend", "old.tsv"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--cluster-fit"] + other)
        assert "--cluster-fit" in capsys.readouterr().err
    assert "--cluster-fit" in cli.build_parser().format_help()
    base = dict(infile="in.tsv", outdir="out", is_genome_dir=False, metric="jc", nr_distance=0.05, nr_linkage="single", clu_distance=0.75,
                clu_linkage="single", sub_distance=0.4, sub_linkage="single", k_min=6, no_sub=False, colors=["red", "white"], midpoint=0.5,
                cpus=1, rm_tmp=False, debug=False, cluster_fit=True)
    for other in (dict(adjacency_only=True), dict(components_only=True), dict(tree=True), dict(nearest=3), dict(extend="old.tsv")):
        with pytest.raises(ValueError, match="cluster_fit"):
            script.phamclust(**base, **other)
