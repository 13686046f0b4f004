"""The tree fill's host side (no GPU): the binding of pc_fill_tree / pc_multi_fill_tree, the key of the total order
(pc_tree_key / pc_tree_key_parts), ``SingleLinkageTree`` against scipy's and scikit-learn's single linkage on every committed
dense fixture, the tie-break stated as a result, and the command line of --tree.

The single-linkage dendrogram is the minimum spanning tree of the complete graph; under one strict total order on the pairs (the
better value, then the smaller target, then the smaller source) it is unique.  ``SingleLinkageTree.from_dense`` states it on the
host; tests/test_gpu_tree.py holds the GPU fill to it."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ALL_METRICS, REPO, golden_file, read_lower_triangle, synth200_file

EPS = (0.25, 0.4, 0.75, 0.999999)                       # the thresholds of tests/test_components_host.py
NEW_EXPORTS = ("pc_fill_tree", "pc_multi_fill_tree", "pc_last_tree_times", "pc_last_tree_rounds", "pc_tree_key", "pc_tree_key_parts")
NONE = 2 ** 64 - 1
MILLION = 10 ** 6

_DENSE = {}


def dense(name, metric):
    """(SymMatrix, condensed vector, SingleLinkageTree.from_dense, scipy's single linkage) of a fixture, computed once."""
    from scipy.cluster.hierarchy import linkage
    from phamclust_amd.matrix import SingleLinkageTree, SymMatrix
    key = (name, metric)
    if key not in _DENSE:
        names, condensed, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
        matrix = SymMatrix.from_condensed(names, condensed, is_distance=True)
        matrix.lock()
        _DENSE[key] = (matrix, condensed, SingleLinkageTree.from_dense(matrix), linkage(condensed, "single"))
    return _DENSE[key]


def same_partition(a, b):
    """Two label vectors describe one partition."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


# ---- binding --------------------------------------------------------------------------------------
def test_tree_fill_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b(int|uint64_t) " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert hip.load().pc_version() >= 161
    assert re.search(r"#define\s+PC_TREE_MAX_GENOMES\s+\(1 << 22\)", header) and hip.Context.TREE_MAX_GENOMES == 1 << 22
    assert hasattr(hip.Context, "fill_tree") and hasattr(hip.MultiContext, "fill_tree")


# ---- the key --------------------------------------------------------------------------------------
def test_key_round_trip_at_the_edges_of_every_field(native_built):
    from phamclust_amd.hip import Context
    top = (1 << 22) - 1
    for micro in (0, 1, MILLION):
        for s, t in ((0, 1), (top - 1, top), (0, top), (5, 6)):
            key = Context.tree_key(micro, s, t)
            assert key == (micro << 44) | (t << 22) | s and key != NONE
            assert Context.tree_key_parts(key) == (micro, s, t)
    assert Context.tree_key_parts(NONE) is None                              # ~0 is no key: its value field is above 10^6
    assert Context.tree_key_parts((MILLION + 1) << 44 | 1 << 22) is None
    assert Context.tree_key_parts(Context.tree_key(3, 7, 9) & ~(0x3FFFFF << 22)) is None          # s >= t
    for bad in ((-1, 0, 1), (MILLION + 1, 0, 1), (0, 1, 1), (0, 2, 1), (0, -1, 1), (0, 0, 1 << 22)):
        assert Context.tree_key(*bad) == NONE


def test_key_order_is_the_total_order(native_built):
    from phamclust_amd.hip import Context
    rng = np.random.default_rng(11)
    micro = rng.integers(0, 6, 4000) * 200000                                # few values: plenty of ties
    t = rng.integers(1, 40, 4000)
    s = (rng.random(4000) * t).astype(np.int64)
    triples = sorted(set(zip(micro.tolist(), t.tolist(), s.tolist())))        # (value, t, s) ascending: the total order
    assert len(triples) > 1500
    shuffled = [triples[i] for i in rng.permutation(len(triples))]
    keys = [Context.tree_key(m, ss, tt) for m, tt, ss in shuffled]
    assert [shuffled[i] for i in np.argsort(np.array(keys, dtype=np.uint64), kind="stable")] == triples
    assert max(keys) < NONE


def test_every_millionth_is_in_the_keys_domain():
    """k -> k / 10^6 -> rint(x * 10^6) is the identity on 0..10^6: the map between delivered values and keys is a bijection."""
    k = np.arange(MILLION + 1, dtype=np.float64)
    assert np.array_equal(np.rint((k / 1e6) * 1e6), k)
    assert np.array_equal(np.round(k / 1e6, 6), k / 1e6)


# ---- from_dense against scipy and scikit-learn, on every dense fixture the reference wrote ----------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_from_dense_is_scipys_single_linkage(name, metric):
    from scipy.cluster.hierarchy import fcluster, is_valid_linkage
    from phamclust_amd.matrix import Components, SparseEdges
    matrix, condensed, tree, z = dense(name, metric)
    n = len(matrix)
    assert len(tree) == n - 1 and tree.is_distance and tree.nodes == matrix.nodes
    assert (tree.source < tree.target).all()
    assert np.array_equal(tree.heights(), z[:, 2])                            # element for element
    # every edge carries the matrix's value, and the edges are in the total order
    full = matrix.to_ndarray()
    assert np.array_equal(tree.weight, full[tree.source, tree.target])
    order = np.lexsort((tree.source, tree.target, tree.weight))
    assert np.array_equal(order, np.arange(n - 1))
    mine = tree.linkage()
    assert mine.shape == (n - 1, 4) and mine.dtype == np.float64 and is_valid_linkage(mine, throw=True)
    assert np.array_equal(mine[:, 2], z[:, 2]) and mine[-1, 3] == n and (mine[:, 0] < mine[:, 1]).all()
    heights = np.unique(z[:, 2])
    picked = heights[np.unique(np.linspace(0, heights.shape[0] - 1, min(12, heights.shape[0])).round().astype(int))].tolist()
    for thr in list(EPS) + picked:
        assert same_partition(fcluster(mine, thr, "distance"), fcluster(z, thr, "distance")), (name, metric, thr)
    every = SparseEdges.from_dense(matrix, 2.0)
    for eps in list(EPS) + picked:
        for strict in (True, False):
            labels = tree.cut(eps, strict=strict)
            assert labels.dtype == np.int32 and np.array_equal(labels, every.components(eps, strict=strict)), (name, metric, eps, strict)
            Components(matrix.nodes, labels)                                  # labels are the smallest member's index
    leaves = tree.leaves()
    assert sorted(leaves) == list(range(n))
    assert [(a, b) for a, b, _ in tree][:3] == [(matrix.nodes[i], matrix.nodes[j]) for i, j in zip(tree.source[:3], tree.target[:3])]


@pytest.mark.parametrize("name", ["small", "synth200"])
def test_cut_n_is_scikit_learns_single_linkage(name, tmp_path):
    """Every metric of the fixture, every k whose two heights at the cut differ (scikit-learn builds one tree per matrix: its
    ``memory`` keeps it between the fits, which changes no result).  The fixture must hold both kinds of cut."""
    from sklearn.cluster import AgglomerativeClustering
    clear, tied = 0, 0
    for metric in ALL_METRICS:
        matrix, condensed, tree, z = dense(name, metric)
        n = len(matrix)
        full = matrix.to_ndarray()
        w = tree.heights()
        for k in range(1, n + 1):
            used = n - k                                                      # merges made; the cut lies between w[used - 1] and w[used]
            differ = not (0 < used < n - 1) or w[used - 1] != w[used]
            tied += not differ
            if not differ:
                continue
            clear += 1
            labels = tree.cut_n(k)
            assert len(set(labels.tolist())) == k
            want = AgglomerativeClustering(n_clusters=k, linkage="single", metric="precomputed", compute_full_tree=True,
                                           memory=str(tmp_path / metric)).fit_predict(full)
            assert same_partition(labels, want), (name, metric, k)
        assert np.array_equal(tree.cut_n(n), np.arange(n)) and not tree.cut_n(1).any()
        for bad in (0, n + 1, 2.0, True):
            with pytest.raises(ValueError):
                tree.cut_n(bad)
    assert clear >= 1 and tied >= 1, (name, clear, tied)


def test_inverted_keeps_the_merge_order():
    from phamclust_amd.matrix import SingleLinkageTree
    matrix, _, tree, _ = dense("synth200", "jc")
    similar = matrix.extract_submatrix(matrix.nodes)
    similar.invert()
    direct = SingleLinkageTree.from_dense(similar)
    turned = tree.inverted()
    assert not turned.is_distance and not direct.is_distance
    assert np.array_equal(direct.source, turned.source) and np.array_equal(direct.target, turned.target)
    assert np.array_equal(direct.weight, turned.weight)
    assert np.array_equal(direct.cut(round(1.0 - 0.75, 6)), tree.cut(0.75))
    with pytest.raises(ValueError, match="distances"):
        turned.linkage()
    back = turned.inverted()
    assert back.is_distance and np.array_equal(back.weight, tree.weight)


# ---- the tie-break, stated as a result --------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 40])
@pytest.mark.parametrize("as_distance", [True, False])
def test_all_values_equal_gives_the_star_at_node_zero(n, as_distance):
    from phamclust_amd.matrix import SingleLinkageTree, SymMatrix
    nodes = [f"n{k:03d}" for k in range(n)]
    matrix = SymMatrix.from_condensed(nodes, np.full(n * (n - 1) // 2, 0.5), is_distance=as_distance)
    tree = SingleLinkageTree.from_dense(matrix)
    assert tree.source.tolist() == [0] * (n - 1) and tree.target.tolist() == list(range(1, n))
    assert (tree.weight == 0.5).all() and tree.is_distance == as_distance
    assert not tree.cut(0.5, strict=False).any() and np.array_equal(tree.cut(0.5), np.arange(n))
    assert tree.cut_n(n - 2).tolist() == [0, 0, 0] + list(range(3, n))


def test_tiny_trees_and_bad_arguments():
    from phamclust_amd.matrix import SingleLinkageTree, SymMatrix
    for n in (0, 1):
        tree = SingleLinkageTree([f"x{k}" for k in range(n)], [], [], [])
        assert len(tree) == 0 and tree.cut(0.5).tolist() == list(range(n)) and tree.leaves() == list(range(n)) and list(tree) == []
        assert tree.linkage().shape == (0, 4)
    two = SingleLinkageTree.from_dense(SymMatrix.from_condensed(["a", "b"], np.array([0.25]), is_distance=True))
    assert list(two) == [("a", "b", 0.25)] and two.linkage().tolist() == [[0.0, 1.0, 0.25, 2.0]] and two.leaves() in ([0, 1], [1, 0])
    for bad in (dict(source=[1], target=[0], weight=[0.1]), dict(source=[0], target=[2], weight=[0.1]), dict(source=[0, 0], target=[1, 1], weight=[0.1, 0.1])):
        with pytest.raises(ValueError):
            SingleLinkageTree(["a", "b"], **bad)


# ---- refusals and the command line -------------------------------------------------------------------------
def test_refusals(monkeypatch, small_genomes):
    from phamclust_amd import cli
    from phamclust_amd.clustering import hierarchical_clustering_de_novo
    from phamclust_amd.matrix import tree_de_novo
    jc = cli.METRICS["jc"]
    with pytest.raises(ValueError, match="no CPU route"):
        tree_de_novo(small_genomes, lambda s, t, as_distance=True: 0.0)
    with pytest.raises(ValueError):
        tree_de_novo([], jc)
    with pytest.raises(ValueError, match="n_clusters.*cut_n"):               # existing behaviour stays; the message points at the tree
        hierarchical_clustering_de_novo(small_genomes, jc, "single", n_clusters=3)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        tree_de_novo(small_genomes, jc)


def test_tree_command_line(capsys):
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--tree"])
    assert args.tree and not args.adjacency_only and args.nearest is None
    assert cli.parse_args(["in.tsv", "out", "-T"]).tree and cli.parse_args(["in.tsv", "out", "-T", "--gpus", "2"]).gpus == 2
    assert not cli.parse_args(["in.tsv", "out"]).tree and cli.DEFAULTS["tree"] is False
    for bad in (["-A"], ["-C"], ["-N"], ["-K", "3"], ["-x", "old.tsv"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--tree"] + bad)
        assert "--tree" in capsys.readouterr().err
    from phamclust_amd.scripts.phamclust import phamclust
    for other in (dict(adjacency_only=True), dict(components_only=True), dict(no_matrix=True), dict(nearest=3), dict(extend="old.tsv")):
        with pytest.raises(ValueError, match="tree"):
            phamclust(None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False, tree=True, **other)
