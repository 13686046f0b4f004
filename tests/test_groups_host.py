"""The groups fill's host side (no GPU): the arithmetic of its domain -- where each group's condensed triangle starts, which 32 x 32
tiles over the groups' members laid end to end hold a pair -- against a brute-force numpy enumeration, the binding of the new
exports, the refusals of ``submatrices_de_novo`` that must fire before any GPU call, and the conflicts of ``--no-matrix``.

tests/test_gpu_groups.py holds the fill itself to the whole fill and the oracle."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_file, read_lower_triangle

TILE = 32
SIZE_LISTS = [[], [0], [1, 1, 1], [2], [31], [32], [33], [65], [30, 5], [2] * 40, [3, 0, 1, 70, 2]]


def random_size_lists():
    rng = np.random.default_rng(158)
    lists = []
    for k in range(200):
        n_groups = int(rng.integers(0, 12))
        top = (4, 40, 100)[k % 3]
        lists.append(rng.integers(0, top + 1, n_groups).tolist())
    return lists


def brute_force(sizes):
    """pair_off and the sorted live tiles by enumerating every slot (p, q), p < q, of every group."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pair_off = np.zeros(len(sizes) + 1, dtype=np.int64)
    tiles = set()
    for c, n in enumerate(sizes):
        pair_off[c + 1] = pair_off[c] + sum(1 for i in range(n) for j in range(i + 1, n))
        if n >= 2:
            p, q = np.triu_indices(n, k=1)
            tiles |= set(zip(((off[c] + p) // TILE).tolist(), ((off[c] + q) // TILE).tolist()))
    return off, pair_off, sorted(tiles)


@pytest.mark.parametrize("sizes", SIZE_LISTS + random_size_lists(), ids=lambda s: "-".join(map(str, s[:6])) + ("+" if len(s) > 6 else "") or "none")
def test_pair_offsets_and_tiles_equal_brute_force(native_built, sizes):
    from phamclust_amd import hip
    off, pair_off, tiles = brute_force(sizes)
    assert np.array_equal(hip.Context.group_pair_offsets(off), pair_off)
    got = hip.Context.group_tiles(off)
    assert got.dtype == np.int32 and got.shape == (len(tiles), 2)
    assert [tuple(t) for t in got.tolist()] == tiles                              # a tile is listed iff a live slot lies in it; sorted by a, then b
    # cap: the count comes back whatever is written, and nothing is written past cap
    lib = hip.load()
    row, col = np.full(3, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    assert lib.pc_group_tiles(off.ctypes.data_as(i64p), len(sizes), row.ctypes.data_as(i32p), col.ctypes.data_as(i32p), 2) == len(tiles)
    assert row[2] == -7 and col[2] == -7
    assert list(zip(row[:2].tolist(), col[:2].tolist()))[:len(tiles)] == tiles[:2]


def test_the_index_of_a_pair_is_scipys_per_group(native_built):
    from scipy.spatial.distance import squareform
    from phamclust_amd import hip
    sizes = [3, 0, 1, 70, 2]
    off, pair_off, _ = brute_force(sizes)
    got = hip.Context.group_pair_offsets(off)
    for c, n in enumerate(sizes):
        assert got[c + 1] - got[c] == n * (n - 1) // 2 == (squareform(np.zeros((n, n))).shape[0] if n else 0)
    # 64-bit: one group of 70,000 genomes exceeds 2^31 pairs
    assert hip.Context.group_pair_offsets([0, 70000, 70003])[1:].tolist() == [70000 * 69999 // 2, 70000 * 69999 // 2 + 3]
    assert 70000 * 69999 // 2 > 2 ** 31


def test_bad_group_offsets_are_refused(native_built):
    from phamclust_amd import hip
    for bad in ([1, 3], [0, 5, 4], [0, 2, 1, 6]):
        with pytest.raises(ValueError):
            hip.Context.group_pair_offsets(bad)
        with pytest.raises(ValueError):
            hip.Context.group_tiles(bad)


def test_fill_groups_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    names = ("pc_fill_groups", "pc_fill_groups_dev", "pc_group_pair_offsets", "pc_group_tiles")
    for name in names:
        assert re.search(r"\b(int|int64_t) %s\s*\(" % name, header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    declared = set(re.findall(r"\b(pc_[a-z0-9_]+)\s*\(", header)) - {"pc_ctx"}
    assert declared == set(hip.EXPORTS)
    assert hip.load().pc_version() >= 158
    assert hasattr(hip.Context, "fill_groups") and hasattr(hip.Context, "fill_groups_dev")
    assert ctypes.sizeof(hip.PcPacked) == 16 + 8 * 8 and ctypes.sizeof(hip.PcStats) == 5 * 8 + 2 * 4 + 4 * 4 + 2 * 8       # layouts unchanged


def test_submatrices_de_novo_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import cli, matrix as M
    jc = cli.METRICS["jc"]
    names = [g.name for g in small_genomes]

    def no_gpu(*args, **kwargs):
        raise AssertionError("a refusal must come before any GPU call")
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes._packed_of", no_gpu)
    with pytest.raises(ValueError, match="METRICS"):
        M.submatrices_de_novo(small_genomes, lambda s, t, as_distance=True: 0.0, [names[:3]])
    with pytest.raises(KeyError, match="no such genome"):
        M.submatrices_de_novo(small_genomes, jc, [names[:3], ["no such genome"]])
    with pytest.raises(ValueError, match="twice"):
        M.submatrices_de_novo(small_genomes, jc, [[names[1], names[4], names[1]]])
    with pytest.raises(ValueError, match="twice"):
        M.submatrices_de_novo(small_genomes, jc, [[2, 5, 2]])
    with pytest.raises(IndexError):
        M.submatrices_de_novo(small_genomes, jc, [[0, len(names)]])
    with pytest.raises(ValueError):
        M.submatrices_de_novo([], jc, [[]])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.submatrices_de_novo(small_genomes, jc, [names[:3]])


def test_no_matrix_command_line():
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--no-matrix"])
    assert args.no_matrix and cli.DEFAULTS["no_matrix"] is False and not cli.parse_args(["in.tsv", "out"]).no_matrix
    for bad in (["--no-matrix", "--adjacency-only"], ["--no-matrix", "--components-only"], ["--no-matrix", "--extend", "old.tsv"],
                ["--no-matrix", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
    from phamclust_amd.scripts.phamclust import phamclust
    with pytest.raises(ValueError, match="no-matrix"):
        phamclust(None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False,
                  adjacency_only=True, no_matrix=True)
    with pytest.raises(ValueError, match="no-matrix"):
        phamclust(None, None, False, "jc", 0.0, "ward", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False, no_matrix=True)
    with pytest.raises(ValueError, match="no-matrix"):
        phamclust(None, None, False, "jc", 0.0, "complete", 0.5, "ward", 0.3, "single", 1, False, None, 0.5, 1, False, False, no_matrix=True)


class DenseFills:
    """Stands in for the GPU context of a --no-matrix run: components and groups fills answered from a dense matrix."""

    def __init__(self, matrix):
        self.matrix, self.full, self.calls = matrix, matrix.to_ndarray(), []

    def fill_components(self, metric, threshold, as_distance=True, strict=True):
        from phamclust_amd.matrix import SparseEdges
        self.calls.append("components")
        return SparseEdges.from_dense(self.matrix, 2.0).components(threshold, strict=strict)

    def fill_edges(self, metric, threshold, as_distance=True, want_stats=False):
        from phamclust_amd.matrix import SparseEdges
        self.calls.append("edges")
        edges = SparseEdges.from_dense(self.matrix, threshold)
        return edges.source, edges.target, edges.weight, {"n_edges": len(edges), "n_slabs": 1}

    def fill_groups(self, metric, groups, as_distance=True, want_stats=False):
        self.calls.append("groups")
        parts = []
        for group in groups:
            group = np.asarray(group, dtype=np.int64)
            assert (np.diff(group) > 0).all(), "a group must be strictly ascending"
            i, j = np.triu_indices(len(group), k=1)
            parts.append(self.full[group[i], group[j]])
        return (parts, {"n_pairs": sum(p.size for p in parts)}) if want_stats else parts


@pytest.mark.parametrize("linkages", [("complete", "average", "0.75", "0.25"), ("single", "single", "0.5", "0.2"), ("average", "complete", "0.6", "0.3")],
                         ids=lambda x: "-".join(x))
def test_no_matrix_pipeline_equals_the_dense_pipeline_on_the_reference_matrix(tmp_path, monkeypatch, linkages):
    """The host half of --no-matrix with no GPU: the fills are answered from the reference's own jc matrix, the dense run reads the
    same matrix from its cache.  Every cluster_* and singletons file must come out byte for byte; the similarities file, the dataset
    heatmap and the matrix cache must not come out at all."""
    import json
    import shutil
    from phamclust_amd.matrix import SparseEdges, SymMatrix
    from phamclust_amd.scripts import phamclust as P
    fixture = json.load(open(os.path.join(GOLDEN, "pipeline_jc", "tree.json")))
    names, condensed, _ = read_lower_triangle(golden_file("jc"))
    matrix = SymMatrix.from_condensed(names, condensed, is_distance=True)
    tsv = os.path.join(GOLDEN, "small_input.tsv")
    argv = ["-m", "jc", "-k", str(fixture["k_min"]), "-t", "1", "-nl", linkages[0], "-cl", linkages[1], "-nr", linkages[2], "-c", linkages[3]]
    dense = tmp_path / "dense"
    cache = dense / fixture["md5_tmp_dir"] / "02_distmats"
    cache.mkdir(parents=True)
    shutil.copy(os.path.join(GOLDEN, "jc_distance_matrix.tsv"), cache / "jc_distance_matrix.tsv")
    P.main([tsv, str(dense)] + argv)
    fills = DenseFills(matrix)
    monkeypatch.setattr(P, "upload_for_fills", lambda genomes, func, caller: (fills, "jc", [g.name for g in genomes], {}))
    monkeypatch.setattr(P, "edges_de_novo", lambda *args, **kwargs: pytest.fail("--no-matrix must fill its edges on the context it uploaded to"))
    sparse = tmp_path / "no_matrix"
    P.main([tsv, str(sparse), "--no-matrix"] + argv)
    assert fills.calls.count("components") == 2 and fills.calls.count("groups") == 3 and fills.calls.count("edges") == 1

    def tree(root):
        return {p.relative_to(root).as_posix(): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file() and ".tmp/" not in p.as_posix()}
    a, b = tree(dense), tree(sparse)
    clustered = [rel for rel in a if rel.startswith(("cluster_", "singletons/"))]
    assert len(clustered) > 20 and any("subcluster_" in rel for rel in clustered) and any(rel.startswith("singletons/") for rel in clustered)
    assert sorted(rel for rel in b if rel.startswith(("cluster_", "singletons/"))) == sorted(clustered)
    assert [rel for rel in clustered if a[rel] != b[rel] and not rel.endswith((".svg", ".html"))] == []
    assert sorted(set(a) - set(b)) == ["jc_heatmap.html", "jc_heatmap.svg", "pairwise_jc_similarities.tsv"] and sorted(set(b) - set(a)) == []
    assert not list(sparse.rglob("*distance_matrix.tsv")) and not list(sparse.rglob("02_distmats"))
    # the adjacency file: the dense run's edges (cluster order there, name order here)
    edges = lambda path: sorted(tuple(sorted(l.split("\t")[:2])) + (l.split("\t")[2],) for l in path.read_text().splitlines())        # noqa: E731
    assert edges(sparse / "pairwise_jc_adjacency.tsv") == edges(dense / "pairwise_jc_adjacency.tsv")
    log = (sparse / "phamclust.log").read_text()
    assert "--no-matrix" in log and "pairwise_jc_similarities.tsv" in log and "are not written" in log
