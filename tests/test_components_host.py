"""The components fill's host side (no GPU): the binding of pc_fill_components, SparseEdges.components / Components against the
reference's clustering of its own dense matrices, cluster_by_component against the dense route, and the command line of
--components-only.

Single linkage cut at eps is exactly the connected components of the graph {d < eps} (scikit-learn's distance_threshold is "at or
above which clusters will not be merged": the comparison is strict), and the average / complete clusters at eps each lie inside
one such component.  Both statements are held here to hierarchical_clustering on every committed dense fixture;
tests/test_gpu_components.py holds the GPU fill to SparseEdges.components."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ALL_METRICS, REPO, golden_file, read_lower_triangle, synth200_file

EPS = (0.25, 0.4, 0.75, 0.999999)
LINKAGES = ("single", "average", "complete")

_DENSE = {}


def dense(name, metric):
    """The reference's distance matrix of a fixture as a locked SymMatrix, and its condensed vector (read once)."""
    from phamclust_amd.matrix import SymMatrix
    key = (name, metric)
    if key not in _DENSE:
        names, condensed, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
        _DENSE[key] = (SymMatrix.from_condensed(names, condensed, is_distance=True), condensed)
        _DENSE[key][0].lock()
    return _DENSE[key]


def node_lists(parts):
    return [part.nodes for part in parts]


# ---- binding --------------------------------------------------------------------------------------
def test_fill_components_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    assert re.search(r"\bint pc_fill_components\s*\(", header) and re.search(r"\bint pc_last_component_times\s*\(", header)
    for name in ("pc_fill_components", "pc_last_component_times"):
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert hip.load().pc_version() >= 157
    assert hasattr(hip.Context, "fill_components")


# ---- the two statements, on every dense fixture the reference wrote ---------------------------------------
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_components_are_the_single_linkage_clusters(name, metric, eps):
    from phamclust_amd.clustering import hierarchical_clustering
    from phamclust_amd.matrix import Components, SparseEdges
    matrix, condensed = dense(name, metric)
    labels = SparseEdges.from_dense(matrix, 2.0).components(eps)
    found = Components(matrix.nodes, labels)
    want = node_lists(hierarchical_clustering(matrix, "single", eps=eps))
    assert found.groups() == want, (name, metric, eps)
    assert found.n_components == len(want) == len(found)
    assert [[matrix.nodes[i] for i in g.tolist()] for g in found.group_indices()] == want
    # labels name the smallest member, and an edge list cut at eps already gives the same components
    for group in found.group_indices():
        assert (labels[group] == group.min()).all()
    assert np.array_equal(SparseEdges.from_dense(matrix, eps).components(eps), labels)
    if not (condensed == eps).any():
        assert np.array_equal(SparseEdges.from_dense(matrix, eps).components(), labels)           # threshold=None: every edge held


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_clustering_by_component_equals_the_dense_route(name, metric, eps, linkage):
    from phamclust_amd.clustering import cluster_by_component, hierarchical_clustering
    from phamclust_amd.matrix import Components, SparseEdges
    matrix, _ = dense(name, metric)
    groups = Components(matrix.nodes, SparseEdges.from_dense(matrix, 2.0).components(eps)).groups()
    got = cluster_by_component(groups, matrix.extract_submatrix, linkage, eps)
    want = hierarchical_clustering(matrix, linkage, eps=eps)
    assert node_lists(got) == node_lists(want), (name, metric, eps, linkage)
    for a, b in zip(got, want):
        assert np.array_equal(a.to_ndarray(), b.to_ndarray())
    assert node_lists(cluster_by_component(groups, matrix.extract_submatrix, linkage, eps, nodes=matrix.nodes)) == node_lists(want)


def test_clustering_by_component_in_another_node_order():
    """Nodes not in name order: the node order must be given, and the parts follow IT."""
    from phamclust_amd.clustering import cluster_by_component, hierarchical_clustering
    from phamclust_amd.matrix import Components, SparseEdges
    matrix, _ = dense("small", "jc")
    order = list(np.random.default_rng(5).permutation(matrix.nodes))
    shuffled = matrix.extract_submatrix(order)
    assert shuffled.nodes == order and order != sorted(order)
    for eps in (0.4, 0.75):
        groups = Components(order, SparseEdges.from_dense(shuffled, 2.0).components(eps)).groups()
        for linkage in LINKAGES:
            want = node_lists(hierarchical_clustering(shuffled, linkage, eps=eps))
            assert node_lists(cluster_by_component(groups, shuffled.extract_submatrix, linkage, eps, nodes=order)) == want
    with pytest.raises(ValueError, match="nodes="):
        cluster_by_component(groups, shuffled.extract_submatrix, "single", 0.75)


# ---- strict against non-strict -------------------------------------------------------------------------
def test_strict_and_non_strict_part_at_every_merge_height():
    """At a single-linkage merge height h some merge happens AT h: '<' leaves its two sides apart, '<=' joins them."""
    from scipy.cluster.hierarchy import linkage
    from phamclust_amd.matrix import Components, SparseEdges
    matrix, condensed = dense("synth200", "jc")
    heights = np.unique(linkage(condensed, "single")[:, 2])[:20]
    assert heights.shape[0] == 20
    edges = SparseEdges.from_dense(matrix, 2.0)
    for h in heights.tolist():
        strict = Components(matrix.nodes, edges.components(h, strict=True)).n_components
        loose = Components(matrix.nodes, edges.components(h, strict=False)).n_components
        assert loose < strict, h
    # the similarity side mirrors it: sim > 1 - h is d < h on 6-place values
    similar = SparseEdges.from_dense(matrix, 2.0).inverted()
    h = float(heights[3])
    assert np.array_equal(similar.components(round(1.0 - h, 6), strict=True), edges.components(h, strict=True))
    assert np.array_equal(similar.components(round(1.0 - h, 6), strict=False), edges.components(h, strict=False))


# ---- Components ---------------------------------------------------------------------------------------
def test_groups_ordering_on_a_hand_made_label_vector():
    from phamclust_amd.matrix import Components
    nodes = list("abcdefghij")
    #         a  b  c  d  e  f  g  h  i  j
    labels = [0, 1, 0, 3, 1, 5, 3, 0, 8, 5]         # {a,c,h} {b,e} {d,g} {f,j} {i}
    found = Components(nodes, labels)
    assert found.n_components == 5
    assert found.groups() == [["a", "c", "h"], ["b", "e"], ["d", "g"], ["f", "j"], ["i"]]      # largest first, equal sizes by smallest member
    assert [g.tolist() for g in found.group_indices()] == [[0, 2, 7], [1, 4], [3, 6], [5, 9], [8]]
    assert Components(nodes, np.arange(10)).groups() == [[x] for x in nodes]
    assert Components(nodes, np.zeros(10, dtype=np.int32)).groups() == [nodes]
    assert Components([], []).groups() == [] and Components([], []).n_components == 0
    for bad in ([0, 2, 2], [0, 0], [1, 1, 1], [0, 0, 1]):                    # above its own index; wrong length; no root; label not a root
        with pytest.raises(ValueError):
            Components(nodes[:3], bad)


# ---- refusals -----------------------------------------------------------------------------------------
def test_refusals(monkeypatch, small_genomes):
    from phamclust_amd import cli
    from phamclust_amd.clustering import cluster_by_component, hierarchical_clustering_de_novo
    from phamclust_amd.matrix import components_de_novo
    jc = cli.METRICS["jc"]
    generic = lambda s, t, as_distance=True: 0.0                             # noqa: E731
    with pytest.raises(ValueError, match="ward"):
        hierarchical_clustering_de_novo(small_genomes, jc, "ward", eps=0.5)
    with pytest.raises(ValueError, match="n_clusters"):
        hierarchical_clustering_de_novo(small_genomes, jc, "single", n_clusters=3)
    with pytest.raises(ValueError):
        hierarchical_clustering_de_novo(small_genomes, jc, "single")
    with pytest.raises(ValueError, match="ward"):
        cluster_by_component([["a"]], None, "ward", 0.5)
    with pytest.raises(ValueError, match="no CPU route"):
        components_de_novo(small_genomes, generic, 0.5)
    with pytest.raises(ValueError, match="no CPU route"):
        hierarchical_clustering_de_novo(small_genomes, generic, "single", eps=0.5)
    with pytest.raises(ValueError):
        components_de_novo([], jc, 0.5)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        components_de_novo(small_genomes, jc, 0.75)
    with pytest.raises(RuntimeError, match="one-GPU"):
        hierarchical_clustering_de_novo(small_genomes, jc, "average", eps=0.75)


# ---- command line -----------------------------------------------------------------------------------
def test_components_only_command_line():
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--components-only"])
    assert args.components_only and args.edge_thresh is None and not args.adjacency_only
    assert cli.parse_args(["in.tsv", "out", "--components-only", "--edge-thresh", "0.25"]).edge_thresh == 0.25
    assert not cli.parse_args(["in.tsv", "out"]).components_only and cli.DEFAULTS["components_only"] is False
    for bad in (["--components-only", "--adjacency-only"], ["--components-only", "--extend", "old.tsv"], ["--edge-thresh", "0.25"],
                ["--components-only", "--edge-thresh", "1.5"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
    from phamclust_amd.scripts.phamclust import phamclust
    with pytest.raises(ValueError):
        phamclust(None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False,
                  adjacency_only=True, components_only=True)
