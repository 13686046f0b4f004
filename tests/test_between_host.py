"""The between-groups table on the host (no GPU): the binding of pc_fill_between, ``GroupLinkage.from_dense`` -- the host statement of
the definition -- against brute force over ``SymMatrix.get_weight`` on every dense golden file the reference wrote, what the class
derives from the table (diameter, means, extremes, a coarser partition, the inverted table, the square, the file), and the refusals
that come before any GPU call.  Every comparison is exact (integers, ``np.array_equal``) but the within-group mean against
``SymMatrix.statistics``, whose left-to-right float sum is allowed its own rounding."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ALL_METRICS, REPO, golden_file, read_lower_triangle, synth200_file

NEW_EXPORTS = ("pc_fill_between", "pc_multi_fill_between", "pc_last_between_times", "pc_between_max_groups", "pc_between_segment")
EMPTY = (0, 0, 2 ** 31 - 1, -1)                      # count, sum, lo, hi of an entry no pair fell into


# ---- binding ------------------------------------------------------------------------------------------------------
def test_between_is_exported_everywhere(native_built):
    from phamclust_amd import hip, matrix
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 164 and hip.load().pc_version() >= 164
    declared = int(re.search(r"#define\s+PC_BETWEEN_MAX_GROUPS\s+(\d+)", header).group(1))
    assert hip.Context.BETWEEN_MAX_GROUPS == hip.load().pc_between_max_groups() == declared == matrix.BETWEEN_MAX_GROUPS >= 2048
    assert hip.Context.between_segment() == hip.load().pc_between_segment() >= 0
    assert hasattr(hip.Context, "fill_between") and hasattr(hip.MultiContext, "fill_between")


@pytest.mark.parametrize("symbol", ["pc_fill_between", "pc_multi_fill_between"])
def test_library_refuses_before_upload(native_built, symbol):
    """No context: a refusal, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    junk_i, junk_l = (ctypes.c_int32 * 1)(1), (ctypes.c_int64 * 1)(1)
    ps, pc = ctypes.cast(junk_l, i64p), ctypes.cast(junk_l, i64p)
    pl, ph = ctypes.cast(junk_i, i32p), ctypes.cast(junk_i, i32p)
    nsl = ctypes.c_int32(5)
    group = (ctypes.c_int32 * 1)(0)
    rc = getattr(lib, symbol)(None, 1, 1, group, 1, 0, ctypes.byref(ps), ctypes.byref(pc), ctypes.byref(pl), ctypes.byref(ph), ctypes.byref(nsl), None)
    assert rc != 0 and symbol.encode() in lib.pc_last_error()
    assert not ps and not pc and not pl and not ph and nsl.value == 0


# ---- the definition against brute force ------------------------------------------------------------------------------
def dense_matrix(name, metric):
    from phamclust_amd.matrix import SymMatrix
    names, condensed, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
    return SymMatrix.from_condensed(names, condensed, is_distance=True)


def partitions(matrix):
    """One group, all singletons, g % 7, blocks of consecutive names, the components at two thresholds."""
    from phamclust_amd.matrix import SparseEdges
    names = matrix.nodes
    n = len(names)
    values = np.sort(matrix.to_ndarray(condensed=True))
    edges = SparseEdges.from_dense(matrix, 2.0)
    out = {"one": [names], "singletons": [[x] for x in names], "mod7": [names[r::7] for r in range(7)],
           "blocks": [names[a:a + 1 + n // 9] for a in range(0, n, 1 + n // 9)]}
    for tag, q in (("cc_low", 0.02), ("cc_mid", 0.35)):
        labels = edges.components(float(values[int(q * (values.shape[0] - 1))]), strict=True)
        roots = sorted(set(labels.tolist()))
        out[tag] = [[names[g] for g in np.flatnonzero(labels == r).tolist()] for r in roots]
    return out


def brute(matrix, groups):
    """{(a, b), a <= b: the millionths of every pair between groups a and b}, by Python loops over get_weight."""
    of = {name: a for a, group in enumerate(groups) for name in group}
    names = matrix.nodes
    lists = {}
    for i, first in enumerate(names):
        for second in names[i + 1:]:
            a, b = sorted((of[first], of[second]))
            w = matrix.get_weight(first, second)
            k = int(round(w * 1000000))
            assert k / 1000000 == w
            lists.setdefault((a, b), []).append(k)
    return lists


def check_against_brute(table, lists, label):
    g = len(table)
    for a in range(g):
        for b in range(a, g):
            got = (table.count(a, b), int(table.sum[a, b]), int(table.lo[a, b]), int(table.hi[a, b]))
            ks = lists.get((a, b))
            want = (len(ks), sum(ks), min(ks), max(ks)) if ks else EMPTY
            assert got == want, (label, a, b)
            assert (table.count(b, a), int(table.sum[b, a]), int(table.lo[b, a]), int(table.hi[b, a])) == want, (label, b, a)
            if ks:
                assert table.mean(a, b) == sum(ks) / (len(ks) * 1000000), (label, a, b)
                low, high = min(ks) / 1000000, max(ks) / 1000000
                assert (table.nearest(a, b), table.farthest(a, b)) == ((low, high) if table.is_distance else (high, low)), (label, a, b)


@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_from_dense_and_what_follows_from_it(tmp_path, name, metric):
    from phamclust_amd.matrix import (GroupLinkage, between_from_file, between_to_file, matrix_from_squareform, matrix_to_squareform,
                                      read_squareform)
    matrix = dense_matrix(name, metric)
    similar = matrix.extract_submatrix(matrix.nodes).invert()
    for tag, groups in partitions(matrix).items():
        label = (name, metric, tag)
        table = GroupLinkage.from_dense(matrix, groups)
        assert table.is_distance and table.sum.dtype == table.cnt.dtype == np.int64 and table.lo.dtype == table.hi.dtype == np.int32, label
        lists = brute(matrix, groups)
        check_against_brute(table, lists, label)
        # the diagonal is the group's own sub-matrix
        for a, group in enumerate(groups):
            sub = matrix.extract_submatrix(group)
            assert table.diameter(a) == sub.diameter, (label, a)
            mean, pairs = sub.statistics[0], len(group) * (len(group) - 1) // 2
            assert abs(table.within_mean(a) - mean) <= pairs * 2.0 ** -53 * abs(mean), (label, a)
            assert table.count(a, a) == pairs, (label, a)
        # a coarser partition
        parts = [list(range(a, min(a + 2, len(groups)))) for a in range(0, len(groups), 2)][::-1]
        coarse = [[x for a in part for x in groups[a]] for part in parts]
        assert table.merged(parts) == GroupLinkage.from_dense(matrix, coarse), label
        # the inverted table is the inverted matrix's
        inverted = table.inverted()
        assert not inverted.is_distance and inverted == GroupLinkage.from_dense(similar, groups), label
        assert inverted.inverted() == table, label
        check_against_brute(inverted, {key: [1000000 - k for k in ks] for key, ks in lists.items()}, label)
        # the square, through the squareform file
        group_names = [f"c{a}" for a in range(len(groups))]
        for kind in ("mean", "nearest", "farthest"):
            for one in (table, inverted):
                square = one.to_symmatrix(group_names, kind)
                assert square.is_distance == one.is_distance and square.nodes == group_names, label
                for a in range(len(groups)):
                    assert square.get_weight(f"c{a}", f"c{a}") == round(one.within_mean(a), 6), (label, a)
                    for b in range(a + 1, len(groups)):
                        assert square.get_weight(f"c{a}", f"c{b}") == round(getattr(one, kind)(a, b), 6), (label, kind, a, b)
                path = matrix_to_squareform(square, tmp_path / "square.tsv")
                rows = list(read_squareform(path))
                assert [row[0] for row in rows] == group_names and np.array_equal(np.array([row[1] for row in rows]), square.to_ndarray()), label
                if tag == "singletons":                                     # (a diagonal of 0.0 or 1.0 throughout: the reader takes it)
                    back = matrix_from_squareform(path)
                    assert back.is_distance == square.is_distance and back.nodes == group_names, label
                    assert np.array_equal(back.to_ndarray(), square.to_ndarray()), label
        # the long-form file
        for one in (table, inverted):
            path = between_to_file(one, group_names, tmp_path / "table.tsv")
            names_back, back = between_from_file(path, groups=groups, is_distance=one.is_distance)
            assert names_back == group_names and back == one, label
            lines = open(path).read().splitlines()
            assert lines[0].split("\t") == ["group_a", "group_b", "count", "mean", "min", "max", "sum"], label
            assert len(lines) == 1 + len(groups) * (len(groups) + 1) // 2, label
            first = lines[1].split("\t")
            if one.count(0, 0):
                assert float(first[3]) == one.mean(0, 0) and int(first[6]) == int(one.sum[0, 0]), label


def test_empty_groups_and_left_out_names():
    from phamclust_amd.matrix import GroupLinkage, SymMatrix
    names = ["a", "b", "c", "d"]
    matrix = SymMatrix.from_condensed(names, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], is_distance=True)
    table = GroupLinkage.from_dense(matrix, [["a", "c"], [], ["d"]])       # b takes no part, group 1 is empty
    assert table.cnt.tolist() == [[1, 0, 2], [0, 0, 0], [2, 0, 0]]
    assert table.sum.tolist() == [[200000, 0, 900000], [0, 0, 0], [900000, 0, 0]]
    assert table.lo.tolist() == [[200000, EMPTY[2], 300000], [EMPTY[2]] * 3, [300000, EMPTY[2], EMPTY[2]]]
    assert table.hi.tolist() == [[200000, -1, 600000], [-1] * 3, [600000, -1, -1]]
    assert table.diameter(2) == 0.0 and table.within_mean(2) == 0.0 and table.inverted().within_mean(2) == 1.0
    with pytest.raises(ValueError):
        table.mean(1, 2)
    with pytest.raises(ValueError):
        table.to_symmatrix(["x", "y", "z"])
    with pytest.raises(ValueError):
        GroupLinkage.from_dense(matrix, [["a"], ["a", "b"]])
    with pytest.raises(ValueError):
        table.inverted().diameter(0)
    with pytest.raises(ValueError):
        table.merged([[0, 1], [1]])
    assert table.merged([[2, 0]]).cnt.tolist() == [[3]] and table.merged([[2, 0]]).sum.tolist() == [[1100000]]


# ---- refusals, before any GPU call ------------------------------------------------------------------------------------
def test_fill_between_refuses_its_arguments_before_the_library():
    from phamclust_amd import hip

    class Packed:
        n_genomes = 4

    ctx = object.__new__(hip.Context)
    ctx._packed, ctx._h, ctx._lib = Packed(), None, None                    # (any library call would fail on None)
    with pytest.raises(ValueError, match="group is None"):
        ctx.fill_between("jc", None)
    with pytest.raises(ValueError, match="3 labels for 4 genomes"):
        ctx.fill_between("jc", [0, 1, 2])


def test_between_de_novo_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import matrix
    from phamclust_amd.cli import METRICS

    def no_gpu(*args, **kwargs):
        raise AssertionError("a GPU call was reached")
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_multi_context", no_gpu)
    names = [g.name for g in small_genomes]
    with pytest.raises(ValueError, match="METRICS"):
        matrix.between_de_novo(small_genomes, lambda a, b: 0.5, [names])
    with pytest.raises(ValueError, match="is in no group"):
        matrix.between_de_novo(small_genomes, METRICS["jc"], [names[1:]])
    with pytest.raises(ValueError, match="is in groups 0 and 1"):
        matrix.between_de_novo(small_genomes, METRICS["jc"], [names, names[:1]])
    with pytest.raises(KeyError):
        matrix.between_de_novo(small_genomes, METRICS["jc"], [names, ["nobody"]])
    with pytest.raises(ValueError, match="groups"):
        matrix.between_de_novo(small_genomes, METRICS["jc"], [names] + [[] for _ in range(matrix.BETWEEN_MAX_GROUPS)])
    with pytest.raises(ValueError, match="groups"):
        matrix.between_de_novo(small_genomes, METRICS["jc"], [])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="launcher"):
        matrix.between_de_novo(small_genomes, METRICS["jc"], [names])


def test_cluster_table_command_line(capsys):
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "--cluster-table", "--no-matrix"])
    assert args.cluster_table and args.no_matrix and cli.DEFAULTS["cluster_table"] is False
    assert cli.parse_args(["in.tsv", "out", "--cluster-table", "--gpus", "2"]).gpus == 2
    assert not cli.parse_args(["in.tsv", "out"]).cluster_table
    for other in (["--adjacency-only"], ["--components-only"], ["--tree"], ["--nearest", "3"], ["--extend", "old.tsv"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--cluster-table"] + other)
        assert "--cluster-table" in capsys.readouterr().err
    assert "--cluster-table" in cli.build_parser().format_help()
    base = dict(infile="in.tsv", outdir="out", is_genome_dir=False, metric="jc", nr_distance=0.05, nr_linkage="single", clu_distance=0.75,
                clu_linkage="single", sub_distance=0.4, sub_linkage="single", k_min=6, no_sub=False, colors=["red", "white"], midpoint=0.5,
                cpus=1, rm_tmp=False, debug=False, cluster_table=True)
    for other in (dict(adjacency_only=True), dict(components_only=True), dict(tree=True), dict(nearest=3), dict(extend="old.tsv")):
        with pytest.raises(ValueError, match="cluster_table"):
            script.phamclust(**base, **other)
