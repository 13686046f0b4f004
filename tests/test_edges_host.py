"""The edge-list fill's host side (no GPU): the binding of pc_fill_edges, the slab cut (Context.edge_slabs), SparseEdges and its
writer against the golden matrices the live reference wrote, and the command line of --adjacency-only.

A SparseEdges taken from a dense matrix must reproduce what the reference derives from that dense matrix: the lines of
matrix_to_adjacency (matrix.py:536-551) restricted to the kept pairs, byte for byte, and SymMatrix.nearest_neighbors
(matrix.py:265-296) for every node.  tests/test_gpu_edges.py holds the GPU fill to the same dense vectors."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ALL_METRICS, REPO, golden_file, read_lower_triangle, synth200_file

PAIR_CAP = 2 ** 31 - 1
# pairs with d <= 0.75 in tests/golden/synth200/ (counted from the reference's files)
SYNTH200_WITHIN_075 = {"gcs": 3898, "jc": 3128, "pocp": 3896, "af": 3881, "aai": 17679, "peq": 3845}

_DENSE = {}


def dense(name, metric):
    """The reference's distance matrix of a fixture as a SymMatrix (read once, never modified: tests invert copies)."""
    from phamclust_amd.matrix import SymMatrix
    key = (name, metric)
    if key not in _DENSE:
        names, condensed, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
        _DENSE[key] = (SymMatrix.from_condensed(names, condensed, is_distance=True), condensed)
        _DENSE[key][0].lock()
    return _DENSE[key]


def thresholds(condensed, tied=True):
    """0.999999 (every non-zero similarity), 0.75, and the most frequent value below 1 -- a tie: '<=' against '<' shows.
    ``tied=False``: the one fixture whose values below 1 are all distinct (the 23-genome peq matrix); its most frequent value is
    then simply another threshold that is itself a value of the matrix."""
    values, counts = np.unique(condensed[condensed < 1.0], return_counts=True)
    tie = float(values[np.argmax(counts)])
    assert counts.max() >= 2 or not tied, "the fixture has no repeated value below 1"
    return [0.999999, 0.75, tie]


def unlocked_copy(matrix):
    return matrix.extract_submatrix(matrix.nodes)


# ---- binding --------------------------------------------------------------------------------------
def test_fill_edges_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    assert re.search(r"\bint pc_fill_edges\s*\(", header)
    assert "pc_fill_edges" in hip.EXPORTS
    for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
        assert hasattr(ctypes.CDLL(lib), "pc_fill_edges"), lib
    assert hip.load().pc_version() >= 156
    assert hasattr(hip.Context, "fill_edges")


# ---- the slab cut ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1000])
def test_edge_slabs_tile_the_targets_within_the_budget(native_built, n):
    from phamclust_amd.hip import Context
    for budget in (8, 8 * 3, 8 * 64, 8 * 300, 8 * 2016, 8 * 2017, 1 << 20, 1 << 40):
        cuts = Context.edge_slabs(n, budget).tolist()
        if n == 0:
            assert cuts == [0]
            continue
        assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts, cuts[1:])), (n, budget, cuts)
        for a, b in zip(cuts, cuts[1:]):
            pairs = sum(range(a, b))                               # target t has t pairs (s, t), s < t
            assert pairs <= budget // 8 or b - a == 1, (n, budget, a, b)
        # greedy: a range ends only where the next target would not fit
        for a, b in zip(cuts, cuts[1:-1]):
            assert sum(range(a, b + 1)) > budget // 8, (n, budget, a, b)
        if budget // 8 >= n * (n - 1) // 2:
            assert len(cuts) == 2


def test_edge_slabs_clamp_at_the_pair_cap(native_built):
    from phamclust_amd.hip import Context
    n = 70000                                                      # 2,449,965,000 pairs: more than one u32-indexed slab
    cuts = Context.edge_slabs(n, 1 << 60).tolist()
    assert len(cuts) > 2 and cuts[0] == 0 and cuts[-1] == n
    for a, b in zip(cuts, cuts[1:]):
        assert (b * (b - 1) - a * (a - 1)) // 2 <= PAIR_CAP
    assert cuts == Context.edge_slabs(n, 8 * PAIR_CAP).tolist()
    with pytest.raises(ValueError):
        Context.edge_slabs(10, 0)


# ---- SparseEdges against the reference's dense matrices -----------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_sparse_edges_reproduce_the_dense_matrix(native_built, tmp_path, name, metric):
    from phamclust_amd.matrix import SparseEdges, edges_to_adjacency, matrix_to_adjacency
    matrix, condensed = dense(name, metric)
    n, pairs = len(matrix), condensed.shape[0]
    full = matrix.to_ndarray()
    slot = {node: k for k, node in enumerate(matrix.nodes)}
    dense_file = tmp_path / "dense.tsv"
    matrix_to_adjacency(matrix, dense_file)
    dense_lines = dense_file.read_bytes().splitlines(keepends=True)
    for thr in thresholds(condensed, tied=(name, metric) != ("small", "peq")):
        edges = SparseEdges.from_dense(matrix, thr)
        want = int((condensed <= thr).sum())
        assert len(edges) == want and 0 < want < pairs, (name, metric, thr)
        if name == "synth200" and thr == 0.75:
            assert want == SYNTH200_WITHIN_075[metric]
        if thr == 0.999999:
            assert want == (pairs - 2220 if name == "synth200" else 134)
        # sorted by target, then source; values are the matrix's
        assert (edges.source < edges.target).all()
        key = edges.target.astype(np.int64) * n + edges.source
        assert (np.diff(key) > 0).all()
        assert np.array_equal(edges.weight, full[edges.source, edges.target])
        assert (edges.weight <= thr).all() and edges.is_distance and edges.threshold == thr
        # the adjacency file: the dense matrix's lines with the failing pairs dropped
        kept = []
        for line in dense_lines:
            s, t, _ = line.decode().rstrip("\n").split("\t")
            if s == t or full[slot[s], slot[t]] <= thr:
                kept.append(line)
        got = tmp_path / "edges.tsv"
        edges_to_adjacency(edges, got)
        assert got.read_bytes() == b"".join(kept), (name, metric, thr)
        assert [f"{s}\t{t}\t{w:.6f}\n".encode() for s, t, w in edges] == kept
        # the C formatter and the Python one agree, with and without skip_zero
        for skip_zero in (False, True):
            a, b = tmp_path / "c.tsv", tmp_path / "py.tsv"
            edges_to_adjacency(edges, a, skip_zero=skip_zero)
            edges_to_adjacency(edges, b, skip_zero=skip_zero, use_lib=False)
            assert a.read_bytes() == b.read_bytes()
        # every node's neighbours, distances and (inverted) similarities
        inverted = edges.inverted()
        similar = unlocked_copy(matrix).invert()
        assert not inverted.is_distance and inverted.threshold == round(1.0 - thr, 6) and len(inverted) == len(edges)
        for node in matrix.nodes:
            assert edges.neighbors(node) == matrix.nearest_neighbors(node, thr), (name, metric, thr, node)
            assert inverted.neighbors(node) == similar.nearest_neighbors(node, round(1.0 - thr, 6)), (name, metric, thr, node, "similarity")
        # densified: the matrix wherever d <= thr, the fill elsewhere
        back = edges.to_symmatrix(1.0).to_ndarray()
        assert np.array_equal(back, np.where(full <= thr, full, 1.0))
    # the pipeline's file: every non-zero similarity
    edges = SparseEdges.from_dense(matrix, 0.999999)
    a, b = tmp_path / "sparse_sim.tsv", tmp_path / "dense_sim.tsv"
    edges_to_adjacency(edges.inverted(), a, skip_zero=True)
    matrix_to_adjacency(unlocked_copy(matrix).invert(), b, skip_zero=True)
    assert a.read_bytes() == b.read_bytes() and a.stat().st_size > 0


def test_the_tie_is_kept_by_less_or_equal():
    """synth200 jc holds 30 pairs at exactly 0.985577: a '<' predicate would lose them all."""
    from phamclust_amd.matrix import SparseEdges
    matrix, condensed = dense("synth200", "jc")
    assert int((condensed == 0.985577).sum()) == 30
    edges = SparseEdges.from_dense(matrix, 0.985577)
    assert int((edges.weight == 0.985577).sum()) == 30 and len(edges) == int((condensed < 0.985577).sum()) + 30


def test_sparse_edges_similarity_side_and_errors():
    from phamclust_amd.matrix import SparseEdges, edges_de_novo
    matrix, condensed = dense("small", "gcs")
    similar = unlocked_copy(matrix).invert()
    edges = SparseEdges.from_dense(similar, 0.25)
    assert not edges.is_distance and len(edges) == int((np.round(1.0 - condensed, 6) >= 0.25).sum()) > 0
    first = next(iter(edges))
    assert first == (matrix.nodes[0], matrix.nodes[0], 1.0)                 # a node's self-edge leads its lines (matrix.py:467-468)
    assert np.array_equal(edges.to_symmatrix(0.0).to_ndarray(), np.where(similar.to_ndarray() >= 0.25, similar.to_ndarray(), 0.0))
    with pytest.raises(KeyError):
        edges.neighbors("no such genome")
    with pytest.raises(ValueError):
        SparseEdges(matrix.nodes, [0, 1], [1], [0.5])
    with pytest.raises(ValueError, match="no CPU route"):
        edges_de_novo([object()], lambda s, t, as_distance=True: 0.0, 0.5)
    with pytest.raises(ValueError):
        edges_de_novo([], None, 0.5)


def test_edges_de_novo_refuses_a_launcher(monkeypatch, small_genomes):
    from phamclust_amd import cli
    from phamclust_amd.matrix import edges_de_novo
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        edges_de_novo(small_genomes, cli.METRICS["jc"], 0.75)


# ---- command line -----------------------------------------------------------------------------------
def test_adjacency_only_command_line():
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--adjacency-only"])
    assert args.adjacency_only and args.edge_thresh is None
    assert cli.parse_args(["in.tsv", "out", "--adjacency-only", "--edge-thresh", "0.25"]).edge_thresh == 0.25
    plain = cli.parse_args(["in.tsv", "out"])
    assert not plain.adjacency_only and plain.edge_thresh is None and cli.DEFAULTS["edge_thresh"] is None
    with pytest.raises(SystemExit):
        cli.parse_args(["in.tsv", "out", "--edge-thresh", "0.25"])
    with pytest.raises(SystemExit):
        cli.parse_args(["in.tsv", "out", "--adjacency-only", "--extend", "old.tsv"])
    with pytest.raises(SystemExit):
        cli.parse_args(["in.tsv", "out", "--adjacency-only", "--edge-thresh", "1.5"])
