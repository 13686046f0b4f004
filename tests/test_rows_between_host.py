"""The rows form of the between-groups fill on the host (no GPU): the binding of pc_fill_rows_between, ``GroupLinkage.extended`` -- the
host statement of a grown table -- held to ``GroupLinkage.from_dense`` of the whole collection, the plain loops of
tests/rows_between_value_cases.py (what the injected-values GPU test compares with) held to ``extended``, the file round trip, and every
refusal that must come before a GPU call."""

import ctypes
import os
import re

import numpy as np
import pytest

import rows_between_value_cases as bv
from conftest import REPO

MILLION = 1000000
EMPTY_LO, EMPTY_HI = 2**31 - 1, -1


# ---- binding ------------------------------------------------------------------------------------------------------
def test_rows_between_is_exported_everywhere(native_built):
    from phamclust_amd import hip, matrix
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    assert re.search(r"\bint pc_fill_rows_between\s*\(", header) and "pc_fill_rows_between" in hip.EXPORTS
    for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
        assert hasattr(ctypes.CDLL(lib), "pc_fill_rows_between"), lib
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 169 and hip.load().pc_version() >= 169
    assert hasattr(hip.Context, "fill_rows_between") and len(hip.load().pc_fill_rows_between.argtypes) == 18
    assert hasattr(matrix, "between_extend") and hasattr(matrix.GroupLinkage, "extended")
    source = open(os.path.join(REPO, "phamclust_amd", "csrc", "pc_fill_slabs.hip")).read()
    assert "has no rows form" not in source and "there is no rows form" not in source


def test_library_refuses_before_upload(native_built):
    """No context: PC_ERR_STATE, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    junk_i, junk_l = (ctypes.c_int32 * 1)(1), (ctypes.c_int64 * 1)(1)
    cells = [ctypes.cast(junk_l if kind is i64p else junk_i, kind) for kind in (i64p, i64p, i32p, i32p)]
    n_slabs = ctypes.c_int32(7)
    group, rows = (ctypes.c_int32 * 2)(0, -1), (ctypes.c_int32 * 1)(1)
    rc = lib.pc_fill_rows_between(None, 1, 1, group, 1, rows, 1, None, None, None, None, 0, *(ctypes.byref(c) for c in cells), ctypes.byref(n_slabs), None)
    assert rc == -3 and b"pc_fill_rows_between: upload first" in lib.pc_last_error()
    assert all(not cell for cell in cells) and n_slabs.value == 0


def test_fill_rows_between_refuses_its_arguments_before_the_library():
    from phamclust_amd import hip

    class Packed:
        n_genomes = 4

    ctx = object.__new__(hip.Context)
    ctx._packed, ctx._h, ctx._lib = Packed(), None, None                    # (any library call would fail on None)
    square = np.zeros((2, 2), dtype=np.int64)
    with pytest.raises(ValueError, match="group is None"):
        ctx.fill_rows_between("jc", None, [0])
    with pytest.raises(ValueError, match="rows is None"):
        ctx.fill_rows_between("jc", [0, 1, 0, 1], None)
    with pytest.raises(ValueError, match="3 labels for 4 genomes"):
        ctx.fill_rows_between("jc", [0, 1, -1], [0])
    with pytest.raises(ValueError, match="4-tuple"):
        ctx.fill_rows_between("jc", [0, 1, 0, 1], [0], seed=(square, square, square))
    with pytest.raises(ValueError, match="4-tuple"):
        ctx.fill_rows_between("jc", [0, 1, 0, 1], [0], seed=(square, square, None, square))
    with pytest.raises(ValueError, match=r"seed lo must be 2 x 2 for 2 groups, not \(3, 3\)"):
        ctx.fill_rows_between("jc", [0, 1, 0, 1], [0], seed=(square, square, np.zeros((3, 3), dtype=np.int32), square))
    with pytest.raises(ValueError, match=r"seed sum must be 3 x 3"):
        ctx.fill_rows_between("jc", [0, 1, 0, 1], [0], n_groups=3, seed=(square, square, square, square))
    with pytest.raises(ValueError, match="n_groups 0"):
        ctx.fill_rows_between("jc", [0, 1, 0, 1], [0], n_groups=0)


# ---- the host statement ---------------------------------------------------------------------------------------------
def random_matrix(n, seed, is_distance):
    from phamclust_amd.symmatrix import _square_matrix
    rng = np.random.default_rng(seed)
    upper = np.triu(rng.integers(0, MILLION + 1, size=(n, n)), 1)
    values = (upper + upper.T).astype(np.float64) / 1.0e6
    np.fill_diagonal(values, 0.0 if is_distance else 1.0)
    names = [f"g{i:03d}" for i in range(n)]
    return names, values, _square_matrix(names, values.copy(), is_distance)


def sub_matrix(names, values, keep, is_distance):
    from phamclust_amd.symmatrix import _square_matrix
    at = [k for k, name in enumerate(names) if name in keep]
    return _square_matrix([names[k] for k in at], values[np.ix_(at, at)].copy(), is_distance)


def grown_partitions(names, seed):
    """(tag, stored groups, grown groups): an empty group, a group made only of new genomes, appended groups, nothing new, everything new."""
    rng = np.random.default_rng(seed)
    n = len(names)
    label = rng.integers(0, 3, size=n)
    new = set(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    grown = [[names[i] for i in range(n) if label[i] == a] for a in range(3)]
    stored = [[x for x in group if names.index(x) not in new] for group in grown]
    out = [("mixed", stored, grown),
           ("empty_group", stored + [[]], grown + [[]]),
           ("appended", stored[:2], [grown[0], grown[1]] + [[x] for x in grown[2]]),
           ("nothing_new", grown, grown),
           ("everything_new", [[], []], grown)]
    only_new = [names[i] for i in sorted(new)]
    rest = [x for x in names if x not in only_new]
    out.append(("new_only_group", [rest[::2], rest[1::2], []], [rest[::2], rest[1::2], only_new]))
    out.append(("some_unlabelled", [rest[2::2], rest[1::2]], [rest[2::2] + only_new[1:], rest[1::2]]))
    return out


@pytest.mark.parametrize("is_distance", [True, False])
@pytest.mark.parametrize("n", [2, 3, 7, 40])
def test_extended_equals_from_dense_of_the_whole_collection(n, is_distance):
    from phamclust_amd.matrix import GroupLinkage
    names, values, matrix = random_matrix(n, 100 + n, is_distance)
    for tag, stored_groups, grown in grown_partitions(names, n):
        kept = {x for group in stored_groups for x in group}
        stored = GroupLinkage.from_dense(sub_matrix(names, values, kept, is_distance), stored_groups) if kept else \
            GroupLinkage(stored_groups, *(np.full((len(stored_groups),) * 2, e) for e in (0, 0, EMPTY_LO, EMPTY_HI)), is_distance=is_distance)
        got = stored.extended(matrix, grown)
        assert got == GroupLinkage.from_dense(matrix, grown), (n, tag)
        assert got.sum.dtype == got.cnt.dtype == np.int64 and got.lo.dtype == got.hi.dtype == np.int32 and got.is_distance == is_distance


def test_extended_refuses_a_moved_and_a_missing_member_and_another_direction():
    from phamclust_amd.matrix import GroupLinkage
    names, values, matrix = random_matrix(9, 5, True)
    stored_groups = [names[0:3], names[3:6]]
    stored = GroupLinkage.from_dense(sub_matrix(names, values, set(names[:6]), True), stored_groups)
    with pytest.raises(ValueError, match=f"stored member '{names[2]}' of group 0 moved to group 1"):
        stored.extended(matrix, [names[0:2], names[2:6] + names[6:]])
    with pytest.raises(ValueError, match=f"stored member '{names[4]}' of group 1 is missing"):
        stored.extended(matrix, [names[0:3] + names[6:], [names[3], names[5]]])
    with pytest.raises(ValueError, match="fewer than the stored table's 2"):
        stored.extended(matrix, [names])
    with pytest.raises(ValueError, match="is in groups 0 and 1"):
        stored.extended(matrix, [names[0:3] + names[6:7], names[3:6] + names[6:7]])
    with pytest.raises(ValueError, match="the matrix holds distances, the stored table similarities"):
        stored.inverted().extended(matrix, [names[0:3] + names[6:], names[3:6]])
    with pytest.raises(KeyError):
        stored.extended(matrix, [names[0:3] + ["nobody"], names[3:6]])
    unset = matrix.copy() if hasattr(matrix, "copy") else None
    if unset is not None:
        unset._data[8, 0] = unset._data[0, 8] = 0.1234565
        with pytest.raises(ValueError, match="no millionth"):
            stored.extended(unset, [names[0:3] + names[6:], names[3:6]])


# ---- the plain loops of the injected-values test, held to extended ----------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65])
def test_the_injected_inputs_loops_are_held_to_extended(n):
    """For every injected input of the small shapes: a symmetric matrix whose query rows are the input's, a stored table over the old
    genomes; stored (+) loops == extended == from_dense.  The slab holds the input's values where live and poison everywhere else."""
    from phamclust_amd.matrix import GroupLinkage
    from phamclust_amd.symmatrix import _square_matrix
    for x in bv.inputs(n) + (bv.inputs(n, all_rows=True) if n == 65 else []):
        rng = np.random.default_rng(n)
        upper = np.triu(rng.integers(0, MILLION + 1, size=(n, n)), 1)
        micro = upper + upper.T
        micro[x.rows, :] = x.micro
        micro[:, x.rows] = x.micro.T
        np.fill_diagonal(micro, 0)
        assert np.array_equal(micro, micro.T), x.tag
        names = [f"g{i:04d}" for i in range(n)]
        values = micro.astype(np.float64) / 1.0e6
        groups = [[names[i] for i in np.flatnonzero(x.label == b)] for b in range(x.n_groups)]
        old = [[name for name in group if not x.is_query[names.index(name)]] for group in groups]
        kept = {name for group in old for name in group}
        stored = GroupLinkage.from_dense(sub_matrix(names, values, kept, True), old) if kept else \
            GroupLinkage(old, *(np.full((x.n_groups,) * 2, e) for e in (0, 0, EMPTY_LO, EMPTY_HI)))
        assert np.array_equal(np.outer(x.old_counts(), x.old_counts())[np.triu_indices(x.n_groups, 1)], stored.cnt[np.triu_indices(x.n_groups, 1)]), x.tag
        want = stored.extended(_square_matrix(names, values, True), groups)
        got = bv.combined((stored.sum, stored.cnt, stored.lo.astype(np.int64), stored.hi.astype(np.int64)), x.table())
        for arr, ref in zip(got, (want.sum, want.cnt, want.lo, want.hi)):
            assert np.array_equal(arr, ref), x.tag
        inverted = bv.combined(tuple(a.astype(np.int64) for a in (stored.inverted().sum, stored.cnt, stored.inverted().lo, stored.inverted().hi)),
                               x.table(as_distance=False))
        for arr, ref in zip(inverted, (want.inverted().sum, want.cnt, want.inverted().lo, want.inverted().hi)):
            assert np.array_equal(arr, ref), (x.tag, "similarity")
        slab, live = x.slab(), x.live()
        assert np.array_equal(np.rint(np.abs(slab[live]) * 1.0e6).astype(np.int64), x.micro[live]) and not (slab[live] == 0.5).any(), x.tag
        assert np.isin(slab[~live], bv.POISON).all() and (~live).any(), x.tag
        seed = x.contract_seed(3)
        assert all(np.array_equal(arr, arr.T) for arr in seed) and np.array_equal(seed[1], stored.cnt), x.tag
        full = seed[1] > 0
        assert (seed[0][full] >= seed[1][full] * seed[2][full]).all() and (seed[0][full] <= seed[1][full] * seed[3][full]).all(), x.tag


def test_the_large_and_refused_inputs():
    x = bv.many_groups_input()
    assert x.n == 4097 and x.n_groups == 2048 and x.table()[1].sum() == 2 * (3 * 4096 - 3) - np.trace(x.table()[1])
    for tag, y, slab, pairs in bv.refused_inputs():
        bad = slab[y.live()]
        micro = np.rint(bad * 1.0e6)
        assert int(((micro < 0) | (micro > MILLION) | (micro / 1.0e6 != bad)).sum()) == pairs, tag


# ---- the route's refusals, before any GPU call ------------------------------------------------------------------------
def test_verify_rows_takes_whole_groups_smallest_first():
    from phamclust_amd.results.linkage import BETWEEN_VERIFY_ALONE, _verify_rows
    members = [[0, 1, 2, 3], [4], [], [5, 6], [7, 8, 9]]
    assert _verify_rows(members, 8) == ([1, 3, 4], [4, 5, 6, 7, 8, 9])
    assert _verify_rows(members, 3) == ([1, 3], [4, 5, 6])
    assert _verify_rows(members, 1) == ([1], [4])
    assert _verify_rows([[0, 1, 2], [3, 4, 5, 6]], 2) == ([0], [0, 1, 2])          # the smallest alone, beyond verify
    assert _verify_rows([list(range(BETWEEN_VERIFY_ALONE + 1))], 8) == ([], [])
    assert _verify_rows([[], []], 8) == ([], [])


def test_between_extend_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import matrix
    from phamclust_amd.cli import METRICS

    def no_gpu(*args, **kwargs):
        raise AssertionError("a GPU call was reached")
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_multi_context", no_gpu)
    names = [g.name for g in small_genomes]
    n = len(names)
    old_groups = [names[0:5], names[5:n - 3]]
    grown = [names[0:5] + names[n - 3:n - 1], names[5:n - 3], names[n - 1:]]
    dense = matrix.SymMatrix(names, is_distance=True)
    rng = np.random.default_rng(0)
    for i in range(n):
        for j in range(i):
            dense.set_weight(names[i], names[j], int(rng.integers(0, MILLION + 1)) / MILLION)
    stored = matrix.GroupLinkage.from_dense(dense, old_groups)
    func = METRICS["jc"]
    with pytest.raises(ValueError, match="METRICS.*GroupLinkage.extended"):
        matrix.between_extend(stored, small_genomes, lambda a, b: 0.5, grown)
    with pytest.raises(ValueError, match="is in no group"):
        matrix.between_extend(stored, small_genomes, func, [grown[0], grown[1]])
    with pytest.raises(ValueError, match="is in groups 0 and 2"):
        matrix.between_extend(stored, small_genomes, func, [grown[0], grown[1], grown[2] + names[:1]])
    with pytest.raises(ValueError, match="groups"):
        matrix.between_extend(stored, small_genomes, func, grown + [[] for _ in range(matrix.BETWEEN_MAX_GROUPS)])
    with pytest.raises(ValueError, match=f"stored member '{names[4]}' of group 0 moved to group 1"):
        matrix.between_extend(stored, small_genomes, func, [names[0:4] + names[n - 3:n - 1], names[4:n - 3], names[n - 1:]])
    with pytest.raises(ValueError, match=f"stored member '{names[4]}' of group 0 is missing"):
        matrix.between_extend(stored, small_genomes[:4] + small_genomes[5:], func, [names[0:4] + names[n - 3:n - 1], names[5:n - 3], names[n - 1:]])
    with pytest.raises(ValueError, match="fewer than the stored table's 2"):
        matrix.between_extend(stored, small_genomes, func, [names])
    wrong = matrix.GroupLinkage([names[0:5], names[5:n - 4]], stored.sum, stored.cnt, stored.lo, stored.hi)
    with pytest.raises(ValueError, match="the stored table counts .* pairs between groups 0 and 1"):
        matrix.between_extend(wrong, small_genomes, func, [names[0:5] + names[n - 4:n - 1], names[5:n - 4], names[n - 1:]])
    with pytest.raises(ValueError, match="stored must be a GroupLinkage"):
        matrix.between_extend(None, small_genomes, func, grown)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="launcher"):
        matrix.between_extend(stored, small_genomes, func, grown)
    monkeypatch.delenv("WORLD_SIZE")
    same = matrix.between_extend(stored, small_genomes[:n - 3], func, old_groups + [[]])      # nothing new: the stored table, no GPU call
    assert np.array_equal(same.sum[:2, :2], stored.sum) and same.cnt[2].tolist() == [0, 0, 0] and same.lo[2, 2] == EMPTY_LO
    monkeypatch.setenv("PHAMCLUST_GPUS", "2")                              # several devices named: still the one-GPU context, never the multi one
    with pytest.raises(AssertionError, match="a GPU call was reached"):
        matrix.between_extend(stored, small_genomes, func, grown)


# ---- the file ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_distance", [True, False])
def test_file_round_trip_of_a_grown_table(tmp_path, is_distance):
    """stored file -> between_from_file with the member lists -> extended -> between_to_file == the file of from_dense, byte for byte."""
    from phamclust_amd.matrix import GroupLinkage, between_from_file, between_to_file
    names, values, matrix = random_matrix(23, 77, is_distance)
    old_groups = [names[0:6], names[6:7], names[7:15]]
    grown = [names[0:6] + names[15:18], names[6:7], names[7:15] + names[18:21], names[21:22], names[22:23]]
    titles = ["cluster_1", "cluster_2", names[6], names[21], names[22]]
    stored = GroupLinkage.from_dense(sub_matrix(names, values, set(names[:15]), is_distance), old_groups)
    between_to_file(stored, ["cluster_1", names[6], "cluster_2"], tmp_path / "stored.tsv")
    read_names, read = between_from_file(tmp_path / "stored.tsv", old_groups, is_distance=is_distance)
    assert read_names == ["cluster_1", names[6], "cluster_2"] and read == stored
    between_to_file(read.extended(matrix, grown), ["cluster_1", names[6], "cluster_2", names[21], names[22]], tmp_path / "grown.tsv")
    del titles
    between_to_file(GroupLinkage.from_dense(matrix, grown), ["cluster_1", names[6], "cluster_2", names[21], names[22]], tmp_path / "whole.tsv")
    assert (tmp_path / "grown.tsv").read_bytes() == (tmp_path / "whole.tsv").read_bytes()


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_grow_table_command_line(capsys):
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "--place", "fit.tsv", "--grow-table", "cluster_table_jc.tsv", "--join-min", "0.4"])
    assert str(args.grow_table) == "cluster_table_jc.tsv" and args.join_min == 0.4
    assert cli.DEFAULTS["grow_table"] is None and cli.DEFAULTS["join_min"] is None and cli.parse_args(["in.tsv", "out"]).grow_table is None
    for argv in (["--grow-table", "t.tsv"], ["--cluster-table", "--grow-table", "t.tsv"], ["--place", "fit.tsv", "--join-min", "0.4"],
                 ["--place", "fit.tsv", "--grow-table", "t.tsv", "--join-min", "1.5"], ["--place", "fit.tsv", "--grow-table", "t.tsv", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + argv)
        err = capsys.readouterr().err
        assert "--grow-table" in err or "--join-min" in err or "--place" in err
    assert "--grow-table" in cli.build_parser().format_help() and "--join-min" in cli.build_parser().format_help()
    base = dict(infile="in.tsv", outdir="out", is_genome_dir=False, metric="jc", nr_distance=0.05, nr_linkage="single", clu_distance=0.75,
                clu_linkage="single", sub_distance=0.4, sub_linkage="single", k_min=6, no_sub=False, colors=["red", "white"], midpoint=0.5,
                cpus=1, rm_tmp=False, debug=False)
    with pytest.raises(ValueError, match="grow_table goes with place"):
        script.phamclust(**base, grow_table="t.tsv")
    with pytest.raises(ValueError, match="join_min goes with grow_table"):
        script.phamclust(**base, place="fit.tsv", join_min=0.5)
