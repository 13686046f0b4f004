"""The rows form of the affinity fill on the host (no GPU): the binding of pc_fill_rows_affinity, ``GroupPlacement.from_dense`` -- the
host statement of the definition, which every GPU test of the call compares with -- held to plain loops, what follows from it
(``GroupAffinity`` when everything is labelled, ``grown_own``, ``inverted``, the file, ``assigned``), and every refusal that must come
before a GPU call."""

import ctypes
import os
import re

import numpy as np
import pytest

import placement_value_cases as pv
from conftest import REPO

MILLION = 1000000
EMPTY_LO, EMPTY_HI = 2**31 - 1, -1


# ---- binding ------------------------------------------------------------------------------------------------------
def test_rows_affinity_is_exported_everywhere(native_built):
    from phamclust_amd import hip, matrix
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    assert re.search(r"\bint pc_fill_rows_affinity\s*\(", header) and "pc_fill_rows_affinity" in hip.EXPORTS
    for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
        assert hasattr(ctypes.CDLL(lib), "pc_fill_rows_affinity"), lib
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 168 and hip.load().pc_version() >= 168
    assert "There is no rows form" not in header
    assert hasattr(hip.Context, "fill_rows_affinity") and len(hip.load().pc_fill_rows_affinity.argtypes) == 25
    for name in ("GroupPlacement", "placement_de_novo", "placement_to_file", "placement_from_file"):
        assert hasattr(matrix, name), name


def test_library_refuses_before_upload(native_built):
    """No context: PC_ERR_STATE, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    junk_i, junk_l = (ctypes.c_int32 * 1)(1), (ctypes.c_int64 * 1)(1)
    kinds = (i64p, i32p, i32p, i32p, i64p, i32p, i32p, i64p, i32p, i32p, i64p, i32p, i32p)
    cells = [ctypes.cast(junk_l if kind is i64p else junk_i, kind) for kind in kinds]
    n_slabs = ctypes.c_int32(7)
    group, rows = (ctypes.c_int32 * 2)(0, -1), (ctypes.c_int32 * 1)(1)
    rc = lib.pc_fill_rows_affinity(None, 1, 1, group, 1, rows, 1, 1, 1, 0, *(ctypes.byref(c) for c in cells), ctypes.byref(n_slabs), None)
    assert rc == -3 and b"pc_fill_rows_affinity: upload first" in lib.pc_last_error()
    assert all(not cell for cell in cells) and n_slabs.value == 0


def test_fill_rows_affinity_refuses_its_arguments_before_the_library():
    from phamclust_amd import hip

    class Packed:
        n_genomes = 4

    ctx = object.__new__(hip.Context)
    ctx._packed, ctx._h, ctx._lib = Packed(), None, None                    # (any library call would fail on None)
    with pytest.raises(ValueError, match="group is None"):
        ctx.fill_rows_affinity("jc", None, [0])
    with pytest.raises(ValueError, match="3 labels for 4 genomes"):
        ctx.fill_rows_affinity("jc", [0, 1, -1], [0])


# ---- the host statement against plain loops ---------------------------------------------------------------------------
def held_to_loops(x, placement):
    want = pv.loops(x.micro, x.label, x.n_groups, x.rows)
    k, g = len(x.rows), x.n_groups
    assert placement.queries == x.queries and placement.is_distance
    assert np.array_equal(placement.table[0], np.array(want["tab_sum"], dtype=np.int64).reshape(k, g)), x.tag
    assert np.array_equal(placement.table[1], np.array(want["tab_lo"], dtype=np.int64).reshape(k, g)), x.tag
    assert np.array_equal(placement.table[2], np.array(want["tab_hi"], dtype=np.int64).reshape(k, g)), x.tag
    own = np.array(want["own"], dtype=np.int64).reshape(k, 3)
    assert np.array_equal(placement.own_sum, own[:, 0]) and np.array_equal(placement.own_lo, own[:, 1]) and np.array_equal(placement.own_hi, own[:, 2]), x.tag
    assert np.array_equal(placement.near_group, np.array(want["near_group"], dtype=np.int64).reshape(3, k)), x.tag
    assert np.array_equal(placement.near_sum, want["near_sum"]) and np.array_equal(placement.near_lo, want["near_lo"]), x.tag
    assert np.array_equal(placement.near_hi, want["near_hi"]), x.tag
    gain = np.array(want["gain"], dtype=np.int64).reshape(x.n, 3)
    for arr, col in zip(placement.gain, gain.T):
        assert np.array_equal(arr, col), x.tag
    assert placement.own_sum.dtype == placement.near_sum.dtype == placement.table[0].dtype == placement.gain[0].dtype == np.int64
    assert placement.own_lo.dtype == placement.near_group.dtype == placement.table[1].dtype == placement.gain[2].dtype == np.int32


def test_from_dense_equals_the_loops_on_random_matrices():
    """-1 labels, empty groups, one group, a query alone in its group, every genome a query, no query."""
    rng = np.random.default_rng(7)
    seen = dict(unlabelled_query=0, empty_group=0, alone=0, none_near=0, gain=0)
    for trial in range(60):
        n = int(rng.integers(1, 14))
        n_groups = int(rng.integers(1, 6))
        label = rng.integers(-1, n_groups, size=n)
        if trial % 7 == 0:
            label[:] = 0
        rows = sorted(rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False).tolist())
        if trial % 5 == 0 and rows:
            label[label == label[rows[0]]] = -1 if label[rows[0]] < 0 else label[rows[0]]
            label[rows[0]] = n_groups - 1
            label[[g for g in range(n) if g != rows[0] and label[g] == n_groups - 1]] = 0 if n_groups > 1 else -1
        pool = None if trial % 3 else (0, 1, 500000, MILLION)
        x = pv.Input(f"random{trial}", pv.symmetric(n, 100 + trial, pool), label, n_groups, rows)
        got = x.expected()
        held_to_loops(x, got)
        sizes = np.bincount(x.label[x.label >= 0], minlength=n_groups)
        seen["unlabelled_query"] += int((x.label[x.rows] < 0).any()) if len(rows) else 0
        seen["empty_group"] += int((sizes == 0).any())
        seen["alone"] += int(any(x.label[r] >= 0 and sizes[x.label[r]] == 1 for r in x.rows))
        seen["none_near"] += int((got.near_group[0] < 0).any()) if len(rows) else 0
        seen["gain"] += int((got.gain[1] != EMPTY_LO).any())
    assert all(count >= 3 for count in seen.values()), seen


@pytest.mark.parametrize("n", [2, 3, 63, 65])
def test_the_injected_inputs_are_held_to_the_loops(n):
    """The inputs the GPU test injects (tests/placement_values_driver.py), at the shapes small enough for the triple loop: their
    expected results are the loops', their slabs are poisoned where nothing may read and hold both zeros."""
    inputs = pv.inputs(n)
    assert len(inputs) >= 30 and {x.n_groups for x in inputs} == set(pv.GROUPS)
    for x in inputs[:: 1 if n < 60 else 4]:
        held_to_loops(x, x.expected())
    for x in inputs:
        slab = x.slab()
        assert slab.shape == (len(x.rows), n) and np.isnan(slab[np.arange(len(x.rows)), x.rows]).all() and np.isnan(slab[:, x.label < 0]).all()
        live = ~np.isnan(slab)
        assert np.array_equal(np.rint(slab[live] * 1.0e6), x.micro[x.rows][live])
        assert (x.label[x.rows] < 0).any() and (x.label[x.rows] >= 0).any()
    few = next(x for x in pv.inputs(65) if x.tag.endswith("alternating_few") and x.n_groups == 3)
    assert np.signbit(few.slab()[few.slab() == 0.0]).any() and not np.signbit(few.slab()[few.slab() == 0.0]).all() and (few.slab() == 1.0).any()
    ties = next(x for x in pv.inputs(65) if x.tag.endswith("alternating_constant") and x.n_groups == 3).expected()
    labelled = ties.query_label >= 0
    assert (ties.near_group[:, ~labelled] == 0).all() and (ties.near_group[:, labelled] == np.where(ties.query_label[labelled] == 0, 1, 0)).all()


def test_the_refused_inputs_count_pairs():
    cases = pv.refused_inputs()
    assert len(cases) == 5 * len(pv.BAD_VALUES) and {c[3] for c in cases} == {1, 2, 6}
    for tag, x, slab, pairs in cases:
        clean = x.slab()
        changed = np.argwhere((slab != clean) & ~(np.isnan(slab) & np.isnan(clean)))
        assert {(min(int(x.rows[r]), int(c)), max(int(x.rows[r]), int(c))) for r, c in changed} .__len__() == pairs, tag


# ---- what follows from the statement ----------------------------------------------------------------------------------------
def labelled_input(n, n_groups, seed, rows):
    label = np.random.default_rng(seed).integers(0, n_groups, size=n)
    return pv.Input(f"labelled{seed}", pv.symmetric(n, seed, None if seed % 2 else (0, 3, 500000, MILLION)), label, n_groups, rows)


@pytest.mark.parametrize("as_distance", [True, False])
def test_everything_labelled_is_group_affinitys_rows(as_distance):
    from phamclust_amd.matrix import GroupAffinity, GroupPlacement
    for seed, (n, n_groups) in enumerate(((1, 1), (2, 1), (9, 3), (40, 7), (33, 40))):
        for rows in ([0], [0, n - 1], list(range(n // 3, n // 3 + 4)), list(range(n))):
            rows = sorted({r for r in rows if r < n})
            x = labelled_input(n, n_groups, seed, rows)
            matrix = x.matrix(as_distance)
            whole = GroupAffinity.from_dense(matrix, x.groups)
            got = GroupPlacement.from_dense(matrix, x.groups, x.queries)
            assert got.is_distance == as_distance
            for name in ("own_sum", "own_lo", "own_hi", "near_sum", "near_lo", "near_hi"):
                assert np.array_equal(getattr(got, name), getattr(whole, name)[x.rows]), (seed, rows, name)
            assert np.array_equal(got.near_group, whole.near_group[:, x.rows]), (seed, rows)
            for mine, theirs in zip(got.table, whole.table):
                assert np.array_equal(mine, theirs[x.rows]), (seed, rows)
            assert np.array_equal(got.nearest_group("nearest"), whole.nearest_group("nearest")[x.rows])
            for kind in ("mean", "nearest", "farthest"):
                assert np.array_equal(got.nearest_value(kind), whole.nearest_value(kind)[x.rows], equal_nan=True), (seed, rows, kind)
            assert np.array_equal(got.counts(), whole.counts()[x.rows])


@pytest.mark.parametrize("as_distance", [True, False])
def test_grown_own_is_the_whole_collections_own(as_distance):
    """GroupAffinity of the old sub-matrix (+) gain == GroupAffinity of the whole matrix, own entries and medoids; queries that stay
    unlabelled change nothing."""
    from phamclust_amd.matrix import GroupAffinity, GroupPlacement
    for seed, (n, n_groups) in enumerate(((6, 2), (25, 4), (40, 9), (31, 1))):
        for rows in ([n - 1], [0, 1, n // 2], list(range(2, n, 3))):
            x = labelled_input(n, n_groups, 50 + seed, rows)
            matrix = x.matrix(as_distance)
            old = [name for name in x.names if name not in set(x.queries)]
            stored = GroupAffinity.from_dense(matrix.extract_submatrix(old), [[name for name in group if name in set(old)] for group in x.groups])
            whole = GroupAffinity.from_dense(matrix, x.groups)
            got = GroupPlacement.from_dense(matrix, x.groups, x.queries)
            grown = got.grown_own(stored)
            assert grown.nodes == whole.nodes and grown.is_distance == as_distance
            assert np.array_equal(grown.own_sum, whole.own_sum) and np.array_equal(grown.own_lo, whole.own_lo) and np.array_equal(grown.own_hi, whole.own_hi), (seed, rows)
            assert grown.medoids() == whole.medoids(), (seed, rows)
            loose = GroupPlacement.from_dense(matrix, [[name for name in group if name in set(old)] for group in x.groups], x.queries)
            assert all((arr == empty).all() for arr, empty in zip(loose.gain, (0, EMPTY_LO, EMPTY_HI)))
            same = loose.grown_own(stored)
            at = [x.names.index(name) for name in old]
            assert np.array_equal(same.own_sum[at], stored.own_sum) and np.array_equal(same.own_lo[at], stored.own_lo)
            with pytest.raises(ValueError, match="want_gain"):
                GroupPlacement.from_dense(matrix, x.groups, x.queries, want_gain=False).grown_own(stored)
            with pytest.raises(ValueError, match="direction"):
                got.grown_own(stored.inverted())
            if n_groups > 1 and len(old) > 1:
                moved = [list(group) for group in stored.groups]
                source = next(b for b, group in enumerate(moved) if group)
                moved[(source + 1) % n_groups].append(moved[source].pop())
                other = GroupAffinity.from_dense(matrix.extract_submatrix(old), moved)
                with pytest.raises(ValueError, match="of the stored partition and in"):
                    got.grown_own(other)
            with pytest.raises(ValueError, match="old genomes"):
                got.grown_own(whole)


def test_inverted_file_and_assigned(tmp_path):
    from phamclust_amd.matrix import GroupPlacement, placement_from_file, placement_to_file
    x = pv.inputs(65)[4]
    got = x.expected()
    similar = GroupPlacement.from_dense(x.matrix(as_distance=False), x.groups, x.queries)
    assert not similar.is_distance and similar == got.inverted() and similar.inverted() == got and got != similar
    assert np.array_equal(similar.near_group, got.near_group)
    full = got.counts() > 0
    assert np.array_equal(similar.table[0][full], (got.counts() * MILLION - got.table[0])[full]) and (similar.table[1][~full] == EMPTY_LO).all()
    assert np.array_equal(similar.gain[1][got.gain_counts() > 0], MILLION - got.gain[2][got.gain_counts() > 0])
    for placement in (got, similar, GroupPlacement.from_dense(x.matrix(), x.groups, x.queries, want_gain=False), GroupPlacement.from_dense(x.matrix(), x.groups, [])):
        path = placement_to_file(placement, str(tmp_path / "placement.tsv"))
        back = placement_from_file(path)
        assert back.table is None and (back.gain is None) == (placement.gain is None)
        back.table = placement.table
        assert back == placement
    with pytest.raises(ValueError, match="no placement file"):
        placement_from_file(os.path.join(REPO, "README.md"))
    # assigned: ties go to the smaller group, the threshold is a similarity, compared in integers
    names = [f"g{i}" for i in range(5)]
    micro = np.array([[0, 0, 0, 200000, 200000], [0, 0, 0, 200000, 400000], [0, 0, 0, 200000, 200000], [200000, 200000, 200000, 0, 0],
                      [200000, 400000, 200000, 0, 0]], dtype=np.int64)
    y = pv.Input("ties", micro, [0, 1, -1, -1, -1], 3, [3, 4])
    tied = y.expected()
    assert tied.assigned("mean") == {"g0003": 0, "g0004": 0} and tied.assigned("nearest") == {"g0003": 0, "g0004": 0}
    assert tied.assigned("farthest", min_similarity=0.8) == {"g0003": 0, "g0004": 0}
    assert tied.assigned("mean", min_similarity=0.800001) == {"g0003": None, "g0004": None}
    assert tied.inverted().assigned("mean", min_similarity=0.8) == {"g0003": 0, "g0004": 0}
    assert tied.inverted().assigned("mean", min_similarity=0.800001) == {"g0003": None, "g0004": None}
    nowhere = pv.Input("nowhere", micro, [-1] * 5, 2, [3, 4]).expected()
    assert nowhere.assigned() == {"g0003": None, "g0004": None} and np.isnan(nowhere.nearest_value("mean")).all()
    with pytest.raises(ValueError, match="kind"):
        tied.assigned("closest")


# ---- refusals, before any GPU call ------------------------------------------------------------------------------------
def test_placement_de_novo_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import matrix
    from phamclust_amd.cli import METRICS

    def no_gpu(*args, **kwargs):
        raise AssertionError("a GPU call was reached")
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_multi_context", no_gpu)
    names = [g.name for g in small_genomes]
    with pytest.raises(ValueError, match="METRICS"):
        matrix.placement_de_novo(small_genomes, lambda a, b: 0.5, [names[:-2]])
    with pytest.raises(ValueError, match="need at least 1 genome"):
        matrix.placement_de_novo([], METRICS["jc"], [[]])
    with pytest.raises(ValueError, match="is in groups 0 and 1"):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2], names[:1]])
    with pytest.raises(KeyError):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2], ["nobody"]])
    with pytest.raises(KeyError):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2]], queries=["nobody"])
    with pytest.raises(IndexError):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2]], queries=[len(names)])
    with pytest.raises(ValueError, match="listed twice"):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2]], queries=[names[-1], len(names) - 1])
    with pytest.raises(ValueError, match="groups"):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2]] + [[] for _ in range(matrix.BETWEEN_MAX_GROUPS)])
    with pytest.raises(ValueError, match="groups"):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="launcher"):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2]])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("PHAMCLUST_GPUS", "2")                              # several devices named: still the one-GPU context, never the multi one
    with pytest.raises(AssertionError, match="a GPU call was reached"):
        matrix.placement_de_novo(small_genomes, METRICS["jc"], [names[:-2]])


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_place_command_line(capsys, tmp_path):
    """--place parses, conflicts with what --grow conflicts with (and with the other stage-2-only modes), stays on one GPU in the GPU
    plan, and every conflict fires before a GPU call."""
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "--place", "cluster_fit_jc.tsv"])
    assert str(args.place) == "cluster_fit_jc.tsv" and cli.DEFAULTS["place"] is None and cli.parse_args(["in.tsv", "out"]).place is None
    assert str(cli.parse_args(["in.tsv", "out", "-P", "f.tsv", "-m", "peq"]).place) == "f.tsv"
    for other in (["--adjacency-only"], ["--components-only"], ["--no-matrix"], ["--tree"], ["--nearest", "3"], ["--extend", "old.tsv"], ["--gpus", "2"],
                  ["--cluster-table"], ["--cluster-fit"], ["--tree", "--grow", "tree_jc.tsv"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--place", "fit.tsv"] + other)
        assert "--place" in capsys.readouterr().err
    assert "--place" in cli.build_parser().format_help()
    assert script.gpus_plan(cli.parse_args(["in.tsv", "out", "--place", "fit.tsv"]), "process", None)[:2] == (1, "one")
    assert "--place" in script.gpus_plan(cli.parse_args(["in.tsv", "out", "--place", "fit.tsv"]), "launcher", None)[2]
    base = dict(infile="in.tsv", outdir="out", is_genome_dir=False, metric="jc", nr_distance=0.05, nr_linkage="single", clu_distance=0.75,
                clu_linkage="single", sub_distance=0.4, sub_linkage="single", k_min=6, no_sub=False, colors=["red", "white"], midpoint=0.5,
                cpus=1, rm_tmp=False, debug=False, place="fit.tsv")
    for other in (dict(adjacency_only=True), dict(components_only=True), dict(no_matrix=True), dict(tree=True), dict(nearest=3), dict(extend="old.tsv"),
                  dict(tree=True, grow="tree.tsv"), dict(nearest=3, grow_nearest="n.tsv"), dict(cluster_table=True), dict(cluster_fit=True)):
        with pytest.raises(ValueError, match="place cannot be combined"):
            script.phamclust(**base, **other)


def test_stored_fit_and_report(tmp_path):
    """The reader of a cluster_fit file and the report's text: from the integers, ``none`` / ``nan`` / 0 where there is no cluster."""
    from phamclust_amd.matrix import GroupPlacement, own_similarity_text, placement_report, stored_fit_from_file
    path = tmp_path / "cluster_fit_jc.tsv"
    path.write_text("genome\tcluster\town_similarity\tnearest_cluster\tnearest_similarity\tsilhouette\tmedoid\n"
                    "g0000\tcluster_1\t0.8\tg0002\t0.8\t0.0\t1\ng0001\tcluster_1\t0.8\tg0002\t0.6\t0.5\t0\ng0002\tg0002\tnan\tcluster_1\t0.7\t0.0\t1\n")
    clusters, groups, own = stored_fit_from_file(path)
    assert clusters == ["cluster_1", "g0002"] and groups == [["g0000", "g0001"], ["g0002"]] and own == {"g0000": "0.8", "g0001": "0.8", "g0002": "nan"}
    micro = np.array([[0, 200000, 200000, 100000, 300000], [200000, 0, 400000, 100000, 1000000], [200000, 400000, 0, 500000, 0],
                      [100000, 100000, 500000, 0, 7], [300000, 1000000, 0, 7, 0]], dtype=np.int64)
    x = pv.Input("report", micro, [0, 0, 1, -1, -1], 2, [0, 2, 3, 4])
    got = x.expected()
    assert own_similarity_text(got, "g0000") == own["g0000"] == own_similarity_text(got.inverted(), "g0000") and own_similarity_text(got, "g0002") == "nan"
    assert own_similarity_text(got, "g0003") == "nan"
    lines = placement_report(got, clusters, ["g0003", "g0004"])
    assert lines == placement_report(got.inverted(), clusters, ["g0003", "g0004"]) and len(placement_report(got, clusters)) == 5
    assert lines[0].split("\t") == ["genome", "mean_cluster", "mean_similarity", "nearest_cluster", "nearest_similarity", "farthest_cluster",
                                    "farthest_similarity", "mean_cluster_size", "nearest_cluster_size", "farthest_cluster_size"]
    assert lines[1] == "g0003\tcluster_1\t0.9\tcluster_1\t0.9\tcluster_1\t0.9\t2\t2\t2"
    assert lines[2] == "g0004\tg0002\t1.0\tg0002\t1.0\tg0002\t1.0\t1\t1\t1"
    alone = GroupPlacement.from_dense(x.matrix(), [[], []], ["g0003"])
    assert placement_report(alone, clusters)[1] == "g0003\tnone\tnan\tnone\tnan\tnone\tnan\t0\t0\t0"
    for text in ("genome\tcluster\n", "genome\tcluster\town_similarity\tnearest_cluster\tnearest_similarity\tsilhouette\tmedoid\ng0\tc\t1\n",
                 path.read_text() + "g0000\tcluster_1\t0.8\tg0002\t0.8\t0.0\t1\n"):
        bad = tmp_path / "bad.tsv"
        bad.write_text(text)
        with pytest.raises(ValueError):
            stored_fit_from_file(bad)
