"""The pair-list fill's host side, without a GPU: the exports, the refusals that come before any GPU call, the command line, the
``--pairs`` parser, and the bound behind ``edges_de_novo(prefilter=True)`` -- a pair's delivered peq similarity never exceeds its
delivered af similarity -- on the CPU oracle over every pair of both fixtures."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO


def test_fill_pairs_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in ("pc_fill_pairs", "pc_fill_pairs_dev", "pc_pair_block"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define PC_VERSION (\d+)", header).group(1)) >= 171 and hip.load().pc_version() >= 171
    assert hip.load().pc_pair_block() == 256
    hooks = ctypes.CDLL(os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so"))
    assert hooks.pc_pair_block() == 256 and hooks.pc_version() >= 171
    assert hasattr(hip.Context, "fill_pairs") and hasattr(hip.Context, "fill_pairs_dev")
    # the binding casts to int32: an index beyond 32 bits must be refused, not wrapped onto a valid genome
    for bad in (([2 ** 32 + 1], [0]), ([0], [-2 ** 32]), ([0.5], [1])):
        with pytest.raises(ValueError, match="32 bits"):
            hip.Context._pair_arrays(*bad)
    src, tgt = hip.Context._pair_arrays(np.array([3, 1], dtype=np.int64), [2, 2 ** 31 - 1])
    assert src.dtype == tgt.dtype == np.int32 and src.tolist() == [3, 1] and tgt.tolist() == [2, 2 ** 31 - 1]
    from phamclust_amd import matrix
    from phamclust_amd.results import pairs
    assert matrix.pairs_de_novo is pairs.pairs_de_novo and hasattr(matrix.SparseEdges, "rescored")


def test_pairs_de_novo_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import cli, hip, matrix as M
    jc = cli.METRICS["jc"]
    names = [g.name for g in small_genomes]

    def no_gpu(*args, **kwargs):
        raise AssertionError("a refusal must come before any GPU call")
    monkeypatch.setattr(hip.Context, "upload", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes._packed_of", no_gpu)
    with pytest.raises(ValueError, match="METRICS"):
        M.pairs_de_novo(small_genomes, lambda s, t, as_distance=True: 0.0, [(names[0], names[1])])
    with pytest.raises(KeyError, match="no such genome"):
        M.pairs_de_novo(small_genomes, jc, [(names[0], names[1]), (names[2], "no such genome")])
    with pytest.raises(IndexError):
        M.pairs_de_novo(small_genomes, jc, [(0, len(names))])
    with pytest.raises(IndexError):
        M.pairs_de_novo(small_genomes, jc, np.array([[0, 1], [-1, 2]]))
    with pytest.raises(ValueError, match="no pair"):
        M.pairs_de_novo(small_genomes, jc, [(0, 1, 2)])
    with pytest.raises(ValueError, match="no pair"):
        M.pairs_de_novo(small_genomes, jc, [names[0]])
    with pytest.raises(ValueError):
        M.pairs_de_novo([], jc, [])
    edges = M.SparseEdges(names[:3] + ["a stranger"], [0, 1], [1, 3], [0.5, 0.5])
    with pytest.raises(KeyError, match="a stranger"):
        edges.rescored(small_genomes, jc)
    for metric in ("gcs", "jc", "pocp", "af", "aai"):                    # prefilter is the af bound of peq and of nothing else
        with pytest.raises(ValueError, match="prefilter"):
            M.edges_de_novo(small_genomes, cli.METRICS[metric], 0.5, prefilter=True)
    with pytest.raises(ValueError, match="prefilter"):
        M.edges_de_novo(small_genomes, lambda s, t, as_distance=True: 0.0, 0.5, prefilter=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.pairs_de_novo(small_genomes, jc, [(0, 1)])
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.edges_de_novo(small_genomes, cli.METRICS["peq"], 0.5, prefilter=True)


def test_pairs_and_prefilter_command_line():
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--pairs", "edges.tsv"])
    assert str(args.pairs) == "edges.tsv" and cli.DEFAULTS["pairs"] is None and cli.parse_args(["in.tsv", "out"]).pairs is None
    args = cli.parse_args(["in.tsv", "out", "-m", "peq", "--adjacency-only", "--edge-thresh", "0.25", "--prefilter"])
    assert args.prefilter and cli.DEFAULTS["prefilter"] is False and not cli.parse_args(["in.tsv", "out"]).prefilter
    for other in (["--adjacency-only"], ["--components-only"], ["--no-matrix"], ["--nearest", "3"], ["--tree"], ["--distribution-only"], ["--distribution"],
                  ["--extend", "old.tsv"], ["--place", "fit.tsv"], ["--cluster-table"], ["--cluster-fit"], ["--gpus", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out", "--pairs", "edges.tsv"] + other)
    for bad in (["--prefilter"], ["--prefilter", "--adjacency-only", "-m", "peq"], ["--prefilter", "--adjacency-only", "-m", "aai", "--edge-thresh", "0.5"],
                ["--prefilter", "--adjacency-only", "-m", "jc", "--edge-thresh", "0.5"], ["--prefilter", "--components-only", "-m", "peq", "--edge-thresh", "0.5"],
                ["--prefilter", "--adjacency-only", "-m", "peq", "--edge-thresh", "0.5", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
    help_text = cli.build_parser().format_help()
    assert "--pairs" in help_text and "--prefilter" in help_text
    from phamclust_amd.scripts.phamclust import phamclust
    base = (None, None, False, "peq", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    for other in (dict(adjacency_only=True), dict(components_only=True), dict(no_matrix=True), dict(tree=True), dict(nearest=3), dict(extend="old.tsv"),
                  dict(distribution_only=True)):
        with pytest.raises(ValueError, match="pairs"):
            phamclust(*base, pairs="edges.tsv", **other)
    with pytest.raises(ValueError, match="prefilter"):
        phamclust(*base, prefilter=True)
    with pytest.raises(ValueError, match="prefilter"):
        phamclust(*base, prefilter=True, adjacency_only=True)
    with pytest.raises(ValueError, match="prefilter"):
        phamclust(None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False,
                  prefilter=True, adjacency_only=True, edge_thresh=0.5)


def test_pairs_file_parser(tmp_path):
    from phamclust_amd.scripts.phamclust import read_pairs_file
    path = tmp_path / "pairs.tsv"
    path.write_text("a\tb\t0.250000\nb\ta\nc c\td\textra\tcolumns\t1\n\na\ta\t1.000000\r\n")
    assert read_pairs_file(path) == [("a", "b"), ("b", "a"), ("c c", "d"), ("a", "a")]
    for bad in ("a\tb\nonly one column\n", "a\tb\n\tb\n", "a\t\n"):
        path.write_text(bad)
        with pytest.raises(ValueError, match="line"):
            read_pairs_file(path)
    path.write_text("")
    assert read_pairs_file(path) == []


@pytest.mark.parametrize("name", ["small", "synth200"])
def test_peq_never_exceeds_af(small_packed, synth200_packed, name):
    """The bound on the oracle alone, over all pairs: peq_sim <= af_sim and peq_dist >= round(1 - af_sim, 6); and at every threshold
    the candidate set of ``edges_de_novo(prefilter=True)`` holds every pair that passes."""
    from oracle import oracle
    from phamclust_amd.results.edges import PREFILTER_SLACK
    packed = small_packed if name == "small" else synth200_packed
    s, t = np.triu_indices(packed.n_genomes, k=1)
    af_sim = np.asarray(oracle.pairs(packed, "af", s, t, False))
    peq_sim = np.asarray(oracle.pairs(packed, "peq", s, t, False))
    peq_dist = np.asarray(oracle.pairs(packed, "peq", s, t, True))
    assert PREFILTER_SLACK == 2e-6
    assert (peq_sim <= af_sim).all() and (peq_dist >= np.round(1.0 - af_sim, 6)).all()
    assert (peq_sim > 0).any() and (peq_sim < af_sim).any()
    for threshold in (0.9, 0.75, 0.5, 0.25):
        candidates = af_sim >= (1.0 - threshold) - PREFILTER_SLACK                       # a distance request d <= threshold
        assert candidates[peq_dist <= threshold].all(), (name, threshold, "distance")
        candidates = af_sim >= threshold - PREFILTER_SLACK                               # a similarity request sim >= threshold
        assert candidates[peq_sim >= threshold].all(), (name, threshold, "similarity")
