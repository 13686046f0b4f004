"""The nearest-neighbours fill's host side (no GPU): ``NearestNeighbors.from_dense`` -- the host statement of pc_fill_nearest's
definition -- against what the LIVE reference's ``SymMatrix.nearest_neighbors(node, 1.0)`` returned for the golden distance files
(tests/golden/nearest/, written by tests/golden/make_nearest.py), the class's other methods against brute force, the binding, and
the command line of ``--nearest``."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, REPO, golden_file, read_lower_triangle, synth200_file

_DENSE, _FIXTURE = {}, {}


def dense(name, metric):
    """The reference's distance matrix of a fixture as a locked SymMatrix (read once)."""
    from phamclust_amd.matrix import SymMatrix
    key = (name, metric)
    if key not in _DENSE:
        names, condensed, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
        _DENSE[key] = SymMatrix.from_condensed(names, condensed, is_distance=True)
        _DENSE[key].lock()
    return _DENSE[key]


def fixture(name):
    if name not in _FIXTURE:
        _FIXTURE[name] = json.load(open(os.path.join(GOLDEN, "nearest", f"{name}.json")))
    return _FIXTURE[name]


def rows_tied_across(matrix, k):
    """Rows whose k-th and (k+1)-th nearest are equally near: there the index rule decides who is listed."""
    from phamclust_amd.matrix import NearestNeighbors
    w = NearestNeighbors.from_dense(matrix, k + 1).weights
    return int((w[:, k - 1] == w[:, k]).sum())


# ---- the definition, against the reference ------------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_from_dense_equals_the_reference_on_small(metric):
    from phamclust_amd.matrix import NearestNeighbors
    matrix, want = dense("small", metric), fixture("small")[metric]
    assert len(matrix) == 23 and set(want) == set(matrix.nodes) and all(len(v) == 22 for v in want.values())
    for k in (1, 5, 22, 40):
        found = NearestNeighbors.from_dense(matrix, k)
        assert found.k == min(k, 22) and len(found) == 23 and found.is_distance
        assert found.indices.dtype == np.int32 and found.weights.dtype == np.float64
        for node in matrix.nodes:
            assert found.neighbors(node) == want[node][:k], (metric, k, node)
            assert found.weights_of(node) == [matrix.get_weight(node, other) for other in want[node][:k]], (metric, k, node)
    assert rows_tied_across(matrix, 5) >= 3, "the fixture no longer holds ties across the 5th place"
    # the similarity side: invert() keeps the order (round(1 - d, 6) is monotone and maps equal distances to equal similarities)
    sim = matrix.extract_submatrix(matrix.nodes)
    sim.invert()
    assert not sim.is_distance
    for k in (5, 22):
        found = NearestNeighbors.from_dense(sim, k)
        assert not found.is_distance
        for node in matrix.nodes:
            assert found.neighbors(node) == want[node][:k], (metric, k, node)
            assert found.weights_of(node) == [sim.get_weight(node, other) for other in want[node][:k]]


def test_from_dense_equals_the_reference_on_synth200():
    from phamclust_amd.matrix import NearestNeighbors
    matrix, want = dense("synth200", "jc"), fixture("synth200")["jc"]
    assert len(matrix) == 200 and set(want) == set(matrix.nodes) and all(len(v) == 16 for v in want.values())
    found = NearestNeighbors.from_dense(matrix, 16)
    for node in matrix.nodes:
        assert found.neighbors(node) == want[node], node
    assert rows_tied_across(matrix, 16) >= 9, "the fixture no longer holds ties across the 16th place"


@pytest.mark.parametrize("name,metric", [("small", "jc"), ("small", "peq"), ("synth200", "jc")])
def test_from_dense_equals_this_packages_nearest_neighbors(name, metric):
    from phamclust_amd.matrix import NearestNeighbors
    matrix = dense(name, metric)
    sim = matrix.extract_submatrix(matrix.nodes)
    sim.invert()
    for m, wide_open in ((matrix, 1.0), (sim, 0.0)):
        for k in (1, 7, len(m) - 1):
            found = NearestNeighbors.from_dense(m, k)
            for node in m.nodes:
                assert found.neighbors(node) == m.nearest_neighbors(node, wide_open)[:k]


def test_from_dense_edge_shapes():
    from phamclust_amd.matrix import NearestNeighbors, SymMatrix
    one = SymMatrix(nodes=["a"], is_distance=True)
    one.set_weight("a", "a", 0.0)
    found = NearestNeighbors.from_dense(one, 3)
    assert found.k == 0 and len(found) == 1 and found.neighbors("a") == [] and list(found) == []
    two = SymMatrix.from_condensed(["a", "b"], np.array([0.25]), is_distance=True)
    found = NearestNeighbors.from_dense(two, 3)
    assert found.k == 1 and list(found) == [("a", "b", 0.25), ("b", "a", 0.25)]
    with pytest.raises(ValueError):
        NearestNeighbors.from_dense(two, 0)
    with pytest.raises(KeyError):
        found.neighbors("c")
    with pytest.raises(ValueError):
        NearestNeighbors(["a", "b"], np.zeros((3, 1)), np.zeros((3, 1)))
    # every weight equal: the smallest indices, whatever the direction
    n = 7
    flat = SymMatrix.from_condensed([f"n{k}" for k in range(n)], np.full(n * (n - 1) // 2, 0.5), is_distance=False)
    found = NearestNeighbors.from_dense(flat, 3)
    assert found.indices.tolist() == [[h for h in range(n) if h != g][:3] for g in range(n)]


# ---- the class ------------------------------------------------------------------------------------------
def test_iteration_and_inverted():
    from phamclust_amd.matrix import NearestNeighbors
    matrix = dense("small", "jc")
    found = NearestNeighbors.from_dense(matrix, 5)
    triples = list(found)
    assert len(triples) == 23 * 5
    assert [t[0] for t in triples] == [node for node in matrix.nodes for _ in range(5)]
    for node in matrix.nodes:
        assert [(t[1], t[2]) for t in triples if t[0] == node] == list(zip(found.neighbors(node), found.weights_of(node)))
    other = found.inverted()
    assert not other.is_distance and found.is_distance and np.array_equal(other.indices, found.indices)
    assert np.array_equal(other.weights, np.round(1.0 - found.weights, 6))
    sim = matrix.extract_submatrix(matrix.nodes)
    sim.invert()
    assert np.array_equal(other.weights, NearestNeighbors.from_dense(sim, 5).weights)
    assert np.array_equal(other.inverted().weights, found.weights)


@pytest.mark.parametrize("name,k", [("small", 1), ("small", 5), ("small", 22), ("synth200", 16)])
def test_to_edges_against_brute_force(name, k):
    from phamclust_amd.matrix import NearestNeighbors, SparseEdges
    matrix = dense(name, "jc")
    found = NearestNeighbors.from_dense(matrix, k)
    listed = {(g, int(h)) for g in range(len(found)) for h in found.indices[g]}
    for mutual in (False, True):
        want = sorted({(max(g, h), min(g, h)) for g, h in listed if not mutual or (h, g) in listed})
        edges = found.to_edges(mutual=mutual)
        assert isinstance(edges, SparseEdges) and edges.is_distance and edges.nodes == matrix.nodes
        assert list(zip(edges.target.tolist(), edges.source.tolist())) == want, (name, k, mutual)
        assert edges.weight.tolist() == [matrix.get_weight(matrix.nodes[s], matrix.nodes[t]) for t, s in want]
    union, both = found.to_edges(), found.to_edges(mutual=True)
    assert len(both) <= len(union) and len(union) + len(both) == len(listed)
    if k == len(found) - 1:
        assert len(both) == len(union) == len(found) * (len(found) - 1) // 2
    else:
        assert len(both) < len(union)


# ---- binding --------------------------------------------------------------------------------------------
def test_fill_nearest_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    assert re.search(r"\bint pc_fill_nearest\s*\(", header) and re.search(r"\bint pc_last_nearest_times\s*\(", header)
    assert int(re.search(r"#define\s+PC_NEAREST_MAX_K\s+(\d+)", header).group(1)) == 64 == hip.Context.NEAREST_MAX_K
    for name in ("pc_fill_nearest", "pc_last_nearest_times"):
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert hip.load().pc_version() >= 159
    assert hasattr(hip.Context, "fill_nearest")


# ---- refusals -------------------------------------------------------------------------------------------
def test_refusals(monkeypatch, small_genomes):
    from phamclust_amd import cli
    from phamclust_amd.matrix import NEAREST_MAX_K, neighbors_de_novo
    jc = cli.METRICS["jc"]
    generic = lambda s, t, as_distance=True: 0.0                             # noqa: E731
    assert NEAREST_MAX_K == 64 == cli.NEAREST_MAX_K
    for bad in (0, -1, 65, 2.5, True, None):
        with pytest.raises(ValueError, match="1..64"):
            neighbors_de_novo(small_genomes, jc, bad)
    with pytest.raises(ValueError, match="no CPU route"):
        neighbors_de_novo(small_genomes, generic, 5)
    with pytest.raises(ValueError):
        neighbors_de_novo([], jc, 5)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        neighbors_de_novo(small_genomes, jc, 5)


# ---- command line ---------------------------------------------------------------------------------------
def test_nearest_command_line():
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--nearest", "5"])
    assert args.nearest == 5 and not args.adjacency_only and not args.components_only and not args.no_matrix and args.edge_thresh is None
    assert cli.parse_args(["in.tsv", "out", "--nearest", "64"]).nearest == 64 and cli.parse_args(["in.tsv", "out", "-K", "1"]).nearest == 1
    assert cli.parse_args(["in.tsv", "out"]).nearest is None and cli.DEFAULTS["nearest"] is None
    for bad in (["--nearest", "0"], ["--nearest", "-3"], ["--nearest", "65"], ["--nearest", "five"], ["--nearest"],
                ["--nearest", "5", "--adjacency-only"], ["--nearest", "5", "--components-only"], ["--nearest", "5", "--no-matrix"],
                ["--nearest", "5", "--extend", "old.tsv"], ["--nearest", "5", "--edge-thresh", "0.25"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)


def test_pipeline_function_refuses_bad_combinations():
    import inspect
    from phamclust_amd.scripts.phamclust import phamclust
    params = list(inspect.signature(phamclust).parameters.values())
    assert params[-1].name == "nearest" and params[-1].default is None
    base = (None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    for bad in (dict(nearest=5, adjacency_only=True), dict(nearest=5, components_only=True), dict(nearest=5, no_matrix=True),
                dict(nearest=5, extend="old.tsv"), dict(nearest=0), dict(nearest=65), dict(nearest=5, edge_thresh=0.25)):
        with pytest.raises(ValueError):                                       # before a file is read or a GPU touched: infile is None
            phamclust(*base, **bad)
