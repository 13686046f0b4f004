"""The surface of ``phamclust_amd.matrix`` after its split into one module per result: every name that was readable from it
stays readable from it, and each module below it imports without torch and without the native library (host only, no GPU)."""

import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every class, function and upper-case constant phamclust_amd.matrix defined before the split, private ones included
SURFACE = [
    "AFFINITY_KINDS", "BETWEEN_MAX_GROUPS", "Components", "GroupAffinity", "GroupLinkage", "LAST_FILL", "MILLION", "NEAREST_MAX_K",
    "NearestNeighbors", "SingleLinkageTree", "SparseEdges", "SymMatrix", "_AFFINITY_COLUMNS", "_CONTEXTS", "_EMPTY_HI", "_EMPTY_LO", "_TEXT_LIB",
    "_de_novo_route", "_diagonal_kind", "_extend_fill", "_extend_plan", "_fill_done", "_get_tree_order", "_group_indices", "_grown_positions",
    "_guard_edges", "_guard_neighbors", "_guard_rows", "_kruskal", "_live_row_pairs", "_metric_name", "_outside_in_index_iterator", "_packed_of",
    "_pairs_adjacency", "_positions_without", "_read_rows", "_row_adjacency", "_slab_fill_context", "_square_matrix", "_text_lib",
    "affinity_de_novo", "affinity_from_file", "affinity_to_file", "between_de_novo", "between_from_file", "between_to_file",
    "calculate_adjacency", "components_de_novo", "components_extend", "components_from_file", "components_to_file", "default_device",
    "edges_de_novo", "edges_extend", "edges_to_adjacency", "get_context", "get_multi_context", "in_process_devices", "matrix_de_novo",
    "matrix_extend", "matrix_from_adjacency", "matrix_from_squareform", "matrix_to_adjacency", "matrix_to_squareform", "merge_edge_lists",
    "nearest_from_file", "nearest_to_file", "neighbors_de_novo", "neighbors_extend", "read_adjacency", "read_squareform",
    "submatrices_de_novo", "tree_de_novo", "tree_extend", "tree_from_file", "tree_to_file", "upload_for_fills",
]

MODULES = ["symmatrix", "routes", "results._common", "results.edges", "results.components", "results.neighbors", "results.tree",
           "results.linkage", "results.affinity"]

_CHILD = """
import sys
import phamclust_amd.{module}
assert "torch" not in sys.modules, "torch was imported"
hip = sys.modules.get("phamclust_amd.hip")
assert hip is None or hip._lib is None, "the native library was loaded"
assert "phamclust_amd.matrix" not in sys.modules, "a module below matrix imported it"
"""


def test_every_name_stays_readable_from_matrix():
    from phamclust_amd import matrix, routes
    missing = [name for name in SURFACE if not hasattr(matrix, name)]
    assert not missing, missing
    assert len(set(SURFACE)) == len(SURFACE) == 77
    assert matrix.LAST_FILL is routes.LAST_FILL and matrix._CONTEXTS is routes._CONTEXTS


@pytest.mark.parametrize("module", MODULES)
def test_module_imports_alone_without_torch_or_the_library(module):
    done = subprocess.run([sys.executable, "-c", _CHILD.format(module=module)], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr
