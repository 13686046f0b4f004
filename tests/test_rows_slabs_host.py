"""Growing a stored sparse result on the host (no GPU): the binding of pc_fill_rows_edges / _components / _tree, the refusals of
edges_extend / components_extend / tree_extend and of --grow, the ``extended`` host statements against ``from_dense`` of the grown
matrix -- the proof the feature rests on, run where it can be run -- the guard, genome removal, and the files' round trip.  Everything
is exact."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden_file, read_lower_triangle

NEW_EXPORTS = ("pc_fill_rows_edges", "pc_fill_rows_components", "pc_fill_rows_tree", "pc_rows_pass_span")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def dense(names, square, is_distance):
    from phamclust_amd.matrix import _square_matrix
    return _square_matrix(names, np.array(square, dtype=np.float64), is_distance)


def wide(is_distance):
    return 2.0 if is_distance else -1.0


# ---- binding ------------------------------------------------------------------------------------------------------
def test_rows_forms_are_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 162 and hip.load().pc_version() >= 162
    for call in ("fill_rows_edges", "fill_rows_components", "fill_rows_tree"):
        assert hasattr(hip.Context, call) and not hasattr(hip.MultiContext, call)              # one-GPU calls
    spans = [hip.Context.rows_pass_span(kind) for kind in hip.Context.ROWS_PASSES]
    assert all(span > 0 and span % 128 == 0 for span in spans) and hip.load().pc_rows_pass_span(3) == 0
    assert hip.Context.rows_slabs(200, 7, 8 * 200) == 7 and hip.Context.rows_slabs(200, 7, 8 * 200 * 3) == 3
    assert hip.Context.rows_slabs(200, 7, 1) == 7 and hip.Context.rows_slabs(200, 7, 8 * 200 * 7) == 1
    with pytest.raises(ValueError):
        hip.Context.rows_slabs(200, 7, 0)


def test_library_refuses_before_upload(native_built):
    """No context: PC_ERR_STATE, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ps, pt, pv = i32p(), i32p(), f64p()
    n64, n32, nsl = ctypes.c_int64(5), ctypes.c_int32(5), ctypes.c_int32(5)
    rows = (ctypes.c_int32 * 1)(0)
    rc = lib.pc_fill_rows_edges(None, 1, 1, 0.5, rows, 1, 0, ctypes.byref(ps), ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(n64), ctypes.byref(nsl), None)
    assert rc != 0 and b"pc_fill_rows_edges: upload first" in lib.pc_last_error() and n64.value == 0 and nsl.value == 0
    nsl.value = 5
    rc = lib.pc_fill_rows_components(None, 1, 1, 0.5, 1, rows, 1, None, 0, ctypes.byref(ps), ctypes.byref(n32), ctypes.byref(n64), ctypes.byref(nsl), None)
    assert rc != 0 and b"pc_fill_rows_components: upload first" in lib.pc_last_error() and n32.value == 0 and nsl.value == 0
    n32.value = nsl.value = 5
    rc = lib.pc_fill_rows_tree(None, 1, 1, rows, 1, None, None, None, 0, 0, ctypes.byref(ps), ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(n32),
                               ctypes.byref(nsl), None)
    assert rc != 0 and b"pc_fill_rows_tree: upload first" in lib.pc_last_error() and n32.value == 0 and nsl.value == 0


# ---- the proof: extended() of the old block is from_dense() of the grown matrix ------------------------------------
def tied_matrix(rng, n, twins):
    """A symmetric matrix of millionths drawn from at most 8 levels, with ``twins`` pairs of identical rows."""
    levels = np.sort(rng.choice(1000001, size=int(rng.integers(1, 9)), replace=False)) / 1000000.0
    square = levels[rng.integers(0, levels.shape[0], size=(n, n))]
    square = np.triu(square, 1)
    square = square + square.T
    for _ in range(twins):
        a, b = rng.choice(n, size=2, replace=False).tolist()
        square[b, :], square[:, b] = square[a, :], square[:, a]
        square[a, b] = square[b, a] = levels[0]
    return square, levels


def new_positions(rng, n, k, where):
    if where == "first":
        return list(range(k))
    if where == "last":
        return list(range(n - k, n))
    if where == "adjacent":
        a = int(rng.integers(0, n - k + 1))
        return list(range(a, a + k))
    return sorted(rng.choice(n, size=k, replace=False).tolist())


@pytest.mark.parametrize("is_distance", [True, False])
@pytest.mark.parametrize("where", ["first", "last", "adjacent", "scattered"])
def test_extended_statements_equal_from_dense_of_the_grown_matrix(where, is_distance):
    from phamclust_amd.matrix import Components, SingleLinkageTree, SparseEdges
    rng = np.random.default_rng({"first": 1, "last": 2, "adjacent": 3, "scattered": 4}[where] * 2 + is_distance)
    seen_k = set()
    for n in range(2, 41):
        for k in sorted({1, n - 1, int(rng.integers(1, n))}):
            seen_k.add((n, k))
            square, levels = tied_matrix(rng, n, twins=int(n > 3) * int(rng.integers(0, 3)))
            np.fill_diagonal(square, 0.0 if is_distance else 1.0)
            names = [f"g{g:03d}" for g in range(n)]
            new = new_positions(rng, n, k, where)
            old = [g for g in range(n) if g not in set(new)]
            whole = dense(names, square, is_distance)
            block = dense([names[g] for g in old], square[np.ix_(old, old)], is_distance)
            rows = square[new]
            label = (where, is_distance, n, new)
            got, want = SingleLinkageTree.from_dense(block).extended(names, new, rows), SingleLinkageTree.from_dense(whole)
            assert got.nodes == want.nodes and got.is_distance == is_distance, label
            assert np.array_equal(got.source, want.source) and np.array_equal(got.target, want.target) and same_bits(got.weight, want.weight), label
            for threshold in {float(levels[0]), float(levels[levels.shape[0] // 2]), float(levels[-1])}:
                got, want = SparseEdges.from_dense(block, threshold).extended(names, new, rows), SparseEdges.from_dense(whole, threshold)
                assert got.nodes == want.nodes and got.threshold == threshold and got.is_distance == is_distance, label
                assert np.array_equal(got.source, want.source) and np.array_equal(got.target, want.target) and same_bits(got.weight, want.weight), label
                for strict in (True, False):
                    stored = Components(block.nodes, SparseEdges.from_dense(block, wide(is_distance)).components(threshold, strict))
                    got = stored.extended(names, new, rows, threshold, is_distance=is_distance, strict=strict)
                    assert np.array_equal(got.labels, SparseEdges.from_dense(whole, wide(is_distance)).components(threshold, strict)), label + (strict,)
    assert (2, 1) in seen_k and (40, 39) in seen_k and (40, 1) in seen_k


def test_extended_statements_refuse_what_cannot_be_grown():
    from phamclust_amd.matrix import Components, SingleLinkageTree, SparseEdges
    tree = SingleLinkageTree(["a", "c"], [0], [1], [0.5])
    rows = np.array([[0.25, 0.0, 0.75]])
    assert list(tree.extended(["a", "b", "c"], [1], rows)) == [("a", "b", 0.25), ("a", "c", 0.5)]
    with pytest.raises(ValueError, match="another order"):
        tree.extended(["c", "b", "a"], [1], rows)
    with pytest.raises(KeyError, match="'c'"):
        tree.extended(["a", "b", "d"], [1], rows)
    with pytest.raises(ValueError, match="distinct"):
        tree.extended(["a", "b", "b", "c"], [1, 2], np.zeros((2, 4)))
    with pytest.raises(ValueError, match="exactly the nodes that are not stored"):
        tree.extended(["a", "b", "c"], [0, 1], np.zeros((2, 3)))
    with pytest.raises(ValueError, match="no threshold"):
        SparseEdges(["a", "c"], [0], [1], [0.5]).extended(["a", "b", "c"], [1], rows)
    grown = Components(["a", "c"], [0, 1]).extended(["a", "b", "c"], [1], rows, 0.5)
    assert grown.labels.tolist() == [0, 0, 2]                               # strict: 0.25 < 0.5 joins a and b; 0.75 does not join c
    assert Components(["a", "c"], [0, 1]).extended(["a", "b", "c"], [1], rows, 0.75, strict=False).labels.tolist() == [0, 0, 0]


def test_merge_of_two_sorted_edge_lists():
    from phamclust_amd.matrix import merge_edge_lists
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 40):
        s, t = np.triu_indices(n, k=1)
        order = np.lexsort((s, t))
        s, t = s[order], t[order]
        w = rng.integers(0, 8, s.shape[0]) / 8.0
        for share in (0.0, 0.3, 1.0):
            first = rng.random(s.shape[0]) < share
            got = merge_edge_lists((s[first], t[first], w[first]), (s[~first], t[~first], w[~first]))
            assert np.array_equal(got[0], s) and np.array_equal(got[1], t) and same_bits(got[2], w)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64


# ---- removal ------------------------------------------------------------------------------------------------------
def test_without():
    from phamclust_amd.matrix import Components, SingleLinkageTree, SparseEdges
    names, condensed, _ = read_lower_triangle(golden_file("jc"))
    n = len(names)
    square = np.zeros((n, n))
    square[np.triu_indices(n, k=1)] = condensed
    square = square + square.T
    whole = dense(names, square, True)
    gone = [names[0], names[7], names[n - 1]]
    keep = [g for g in range(n) if names[g] not in gone]
    rest = dense([names[g] for g in keep], square[np.ix_(keep, keep)], True)
    got, want = SparseEdges.from_dense(whole, 0.75).without(gone), SparseEdges.from_dense(rest, 0.75)
    assert got.nodes == want.nodes and np.array_equal(got.source, want.source) and np.array_equal(got.target, want.target)
    assert same_bits(got.weight, want.weight) and got.threshold == 0.75
    with pytest.raises(KeyError):
        SparseEdges.from_dense(whole, 0.75).without(["nobody"])
    labels = SparseEdges.from_dense(whole, 2.0).components(0.75)
    got = Components(names, labels).without(gone)
    assert got.nodes == rest.nodes
    assert np.array_equal(Components(names, labels).without([]).labels, labels)
    for a in range(len(keep)):                                               # the stored partition, restricted; labels the smallest member kept
        assert got.labels[a] == min(b for b in range(len(keep)) if labels[keep[b]] == labels[keep[a]])
    # a path a - b - c: without b the partition still holds a and c together (the labels do not say which pairs were edges) ...
    path = Components(["a", "b", "c"], [0, 0, 0]).without(["b"])
    assert path.nodes == ["a", "c"] and path.labels.tolist() == [0, 0]
    # ... the edge list knows better
    assert SparseEdges(["a", "b", "c"], [0, 1], [1, 2], [0.1, 0.1], threshold=0.5).without(["b"]).components().tolist() == [0, 1]
    with pytest.raises(NotImplementedError, match="not closed under vertex deletion"):
        SingleLinkageTree.from_dense(whole).without(gone)


# ---- the calls' refusals, all before a GPU call ---------------------------------------------------------------------
def _stored(small_genomes, drop):
    from phamclust_amd.matrix import Components, SingleLinkageTree, SparseEdges
    names, condensed, _ = read_lower_triangle(golden_file("jc"))
    assert names == [g.name for g in small_genomes]
    n = len(names)
    square = np.zeros((n, n))
    square[np.triu_indices(n, k=1)] = condensed
    square = square + square.T
    keep = [g for g in range(n) if g not in drop]
    block = dense([names[g] for g in keep], square[np.ix_(keep, keep)], True)
    whole = dense(names, square, True)
    return (SparseEdges.from_dense(block, 0.75), Components(block.nodes, SparseEdges.from_dense(block, 2.0).components(0.75)),
            SingleLinkageTree.from_dense(block)), whole, square


def test_extend_calls_refuse_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    jc = cli.METRICS["jc"]
    (edges, comps, tree), whole, _ = _stored(small_genomes, {3, 4})
    other = lambda s, t, as_distance=True: 0.0                                # noqa: E731
    calls = ((M.edges_extend, edges, ()), (M.components_extend, comps, (0.75,)), (M.tree_extend, tree, ()))
    for call, stored, extra in calls:
        with pytest.raises(ValueError, match="no CPU route"):
            call(stored, small_genomes, other, *extra)
        with pytest.raises(ValueError):
            call(stored, [], jc, *extra)
        with pytest.raises(KeyError, match="is not among the genomes"):
            call(stored, small_genomes[1:], jc, *extra)                      # stored node 0 is no genome
        with pytest.raises(ValueError, match="another order"):
            call(stored, small_genomes[::-1], jc, *extra)
        with pytest.raises(ValueError, match="distinct"):
            call(stored, small_genomes + small_genomes[:1], jc, *extra)
    with pytest.raises(ValueError, match="no threshold"):
        M.edges_extend(M.SparseEdges(edges.nodes, edges.source, edges.target, edges.weight), small_genomes, jc)
    monkeypatch.setenv("WORLD_SIZE", "2")
    for call, stored, extra in calls:
        with pytest.raises(RuntimeError, match="one-GPU"):
            call(stored, small_genomes, jc, *extra)


def test_nothing_new_returns_the_stored_result_relaid(small_genomes):
    """No new genome: no fill, no GPU -- the stored result on the genomes' names."""
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    jc = cli.METRICS["jc"]
    (edges, comps, tree), _, _ = _stored(small_genomes, set())
    got = M.tree_extend(tree, small_genomes, jc)
    assert got.nodes == tree.nodes and np.array_equal(got.source, tree.source) and same_bits(got.weight, tree.weight)
    got = M.edges_extend(edges, small_genomes, jc)
    assert np.array_equal(got.source, edges.source) and np.array_equal(got.target, edges.target) and got.threshold == edges.threshold
    assert np.array_equal(M.components_extend(comps, small_genomes, jc, 0.75).labels, comps.labels)


# ---- the guard (host route: the checks the calls make, on refilled rows computed here) ----------------------------------
def test_guard_raises_on_the_verified_rows(small_genomes):
    from phamclust_amd import matrix as M
    (edges, comps, tree), whole, square = _stored(small_genomes, {3, 4})
    names = whole.nodes
    old_at = np.asarray([g for g in range(len(names)) if g not in (3, 4)], dtype=np.int64)
    checked = [int(g) for g in old_at]                                        # every old genome verified
    values = square[checked]
    for stored, what in ((tree, "tree"), (edges, "edge list")):
        src, tgt = old_at[stored.source], old_at[stored.target]
        M._guard_edges(names, "jc", checked, values, src, tgt, stored.weight, what)            # the true file passes
        off = stored.weight.copy()
        off[len(off) // 2] = round(off[len(off) // 2] + 1e-6, 6)              # a stored value off by one millionth
        with pytest.raises(ValueError, match=f"the {what} holds"):
            M._guard_edges(names, "jc", checked, values, src, tgt, off, what)
        _, other, _ = read_lower_triangle(golden_file("gcs"))                # another metric's file
        other_square = np.zeros_like(square)
        other_square[np.triu_indices(len(names), k=1)] = other
        other_square = other_square + other_square.T
        with pytest.raises(ValueError, match="was not filled with this metric"):
            M._guard_edges(names, "jc", checked, other_square[checked], src, tgt, stored.weight, what)
        # a permuted node order: the stored indices name other genomes
        swapped = old_at.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        with pytest.raises(ValueError, match=f"the {what} holds"):
            M._guard_edges(names, "jc", checked, values, swapped[stored.source], swapped[stored.target], stored.weight, what)


# ---- files --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_files_round_trip_bit_for_bit(metric, tmp_path):
    from phamclust_amd import matrix as M
    names, condensed, _ = read_lower_triangle(golden_file(metric))
    whole = M.SymMatrix.from_condensed(names, condensed, is_distance=True)
    tree = M.SingleLinkageTree.from_dense(whole)
    path = M.tree_to_file(tree, tmp_path / f"tree_{metric}.tsv")
    assert open(path).read() == "".join(f"{s}\t{t}\t{w:.6f}\n" for s, t, w in tree.inverted())   # the bytes --tree has always written
    back = M.tree_from_file(path, names)
    assert back.nodes == tree.nodes and back.is_distance
    assert np.array_equal(back.source, tree.source) and np.array_equal(back.target, tree.target) and same_bits(back.weight, tree.weight)
    sub = M.tree_from_file(path, ["zz_before"] + names + ["zz_after"])         # a longer genome list: the file's names only
    assert sub.nodes == tree.nodes and np.array_equal(sub.source, tree.source)
    with pytest.raises(KeyError):
        M.tree_from_file(path, names[1:])
    with pytest.raises(ValueError, match="another order"):
        M.tree_from_file(path, names[::-1])
    comps = M.Components(names, M.SparseEdges.from_dense(whole, 2.0).components(0.75))
    path = M.components_to_file(comps, tmp_path / f"components_{metric}.tsv")
    number = {}
    for k, group in enumerate(comps.groups(), start=1):
        number.update({name: k for name in group})
    assert open(path).read() == "".join(f"{name}\t{number[name]}\n" for name in names)
    back = M.components_from_file(path)
    assert back.nodes == comps.nodes and np.array_equal(back.labels, comps.labels)


# ---- the command line ---------------------------------------------------------------------------------------------
def test_grow_command_line(capsys):
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--tree", "--grow", "tree_jc.tsv"])
    assert args.tree and str(args.grow) == "tree_jc.tsv" and cli.DEFAULTS["grow"] is None
    args = cli.parse_args(["in.tsv", "out", "--components-only", "--edge-thresh", "0.3", "-w", "components_jc.tsv"])
    assert args.components_only and str(args.grow) == "components_jc.tsv" and cli.parse_args(["in.tsv", "out"]).grow is None
    for bad in (["--grow", "f"], ["--grow", "f", "--adjacency-only"], ["--grow", "f", "--no-matrix"], ["--grow", "f", "--nearest", "3"],
                ["--grow", "f", "--extend", "old.tsv"], ["--grow", "f", "--components-only"], ["--grow", "f", "--tree", "--gpus", "2"],
                ["--grow", "f", "--tree", "--adjacency-only"], ["--grow", "f", "--tree", "--components-only", "-e", "0.3"],
                ["--grow", "f", "--tree", "--extend", "old.tsv"], ["--grow", "f", "--components-only", "-e", "0.3", "--gpus", "4"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
        err = capsys.readouterr().err
        assert "--grow" in err or "--tree stops after a tree fill of its own" in err                # (--tree's own refusals come first)
    # the old --extend conflicts are still refused
    for bad in (["--tree", "--extend", "old.tsv"], ["--components-only", "--extend", "old.tsv"], ["--adjacency-only", "--extend", "old.tsv"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
    base = (None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    for other in (dict(), dict(adjacency_only=True), dict(tree=True, components_only=True, edge_thresh=0.3), dict(tree=True, extend="old.tsv"),
                  dict(components_only=True), dict(tree=True, nearest=3), dict(no_matrix=True)):
        with pytest.raises(ValueError):
            script.phamclust(*base, grow="f", **other)
    plan = script.gpus_plan(cli.parse_args(["in.tsv", "out", "--tree", "--grow", "f"]), "process", None)
    assert plan[:2] == (1, "one") and "one-GPU call" in plan[2]
    assert "--grow" in cli.build_parser().format_help() and "edges_extend" in cli.build_parser().format_help()
