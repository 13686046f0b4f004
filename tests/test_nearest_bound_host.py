"""The bounded nearest fill's host side, without a GPU: ``SparseEdges.nearest`` -- the host statement of pc_nearest_of_pairs -- against
``NearestNeighbors.from_dense`` and a plain-Python statement; the five-step rule of ``_bounded_peq_nearest`` in numpy over the golden
af and peq matrices, which must reproduce ``from_dense`` exactly; where the fallback cap lands; the command line of ``--af-bound``;
the refusals that come before any library call; the header."""

import ctypes
import os
import re

import numpy as np
import pytest

import nearest_bound_cases as NB
from conftest import ALL_METRICS, REPO
from test_nearest_host import dense

NEW_EXPORTS = ("pc_fill_edges_bars", "pc_nearest_of_pairs")
KS = (1, 4, 16, 64)
# candidates of the rule with the af DISTANCE as the bound and no slack, distance direction (the measurement the route was proposed
# on): the route's candidates, taken at the similarity bound less the slack, are a superset
PROPOSED = {"synth200": {1: 1558, 4: 2393, 16: 3380, 64: 13773}, "small": {1: 93, 4: 126, 16: 253, 64: 253}}


def squares(name, as_distance):
    """(af similarity square, peq square in the call's direction) of a fixture; similarities as ``SymMatrix.invert`` makes them."""
    af, peq = dense(name, "af").to_ndarray(), dense(name, "peq").to_ndarray()
    af_sim = np.round(1.0 - af, 6)
    np.fill_diagonal(af_sim, 1.0)
    if not as_distance:
        peq = np.round(1.0 - peq, 6)
    return af_sim, peq


def whole_edges(matrix):
    from phamclust_amd.matrix import SparseEdges
    return SparseEdges.from_dense(matrix, 2.0 if matrix.is_distance else -1.0)


@pytest.mark.parametrize("name, metric", [("small", metric) for metric in ALL_METRICS] + [("synth200", "jc"), ("synth200", "peq")])
def test_nearest_of_a_whole_list_is_from_dense(name, metric):
    from phamclust_amd.matrix import NearestNeighbors
    matrix = dense(name, metric)
    n = len(matrix)
    for sim in (False, True):
        if sim:
            matrix = matrix.extract_submatrix(matrix.nodes)
            matrix.invert()
        edges = whole_edges(matrix)
        assert len(edges) == n * (n - 1) // 2
        for k in (1, 5, 64, n - 1):
            indices, weights, count = edges.nearest(k)
            want = NearestNeighbors.from_dense(matrix, k)
            assert indices.dtype == np.int32 and weights.dtype == np.float64 and count.dtype == np.int32
            assert np.array_equal(indices, want.indices) and np.array_equal(weights.view(np.uint64), want.weights.view(np.uint64))
            assert (count == n - 1).all()


def test_nearest_of_a_sparse_list_pads_and_counts():
    from phamclust_amd.matrix import SparseEdges
    rng = np.random.default_rng(3)
    n = 40
    for as_distance in (True, False):
        t, s = np.tril_indices(n, k=-1)
        keep = rng.random(s.shape[0]) < 0.15
        keep[(s == 7) | (t == 7)] = False                                # a node without an edge
        s, t = s[keep], t[keep]
        w = rng.integers(0, 6, s.shape[0]) / 1000000.0                   # many equal values: the index decides
        edges = SparseEdges([f"g{i}" for i in range(n)], s, t, w, is_distance=as_distance)
        for k in (1, 3, 39, 64):
            got = edges.nearest(k)
            want = NB.nearest_of_pairs(n, s, t, w, k, as_distance)
            assert got[0].shape == (n, min(k, n - 1))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
            assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))       # (the padding is the same quiet NaN)
            assert got[2][7] == 0 and (got[0][7] == -1).all() and np.isnan(got[1][7]).all()
            short = got[2] < got[0].shape[1]
            assert short.any() and all((got[0][g, got[2][g]:] == -1).all() and (got[0][g, :got[2][g]] >= 0).all() for g in np.flatnonzero(short))
    empty = SparseEdges(["a", "b", "c"], [], [], [])
    indices, weights, count = empty.nearest(5)
    assert indices.shape == (3, 2) and (indices == -1).all() and np.isnan(weights).all() and count.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        empty.nearest(0)


@pytest.mark.parametrize("as_distance", [True, False], ids=["distance", "similarity"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_the_rule_reproduces_from_dense(name, k, as_distance):
    af_sim, peq = squares(name, as_distance)
    n = af_sim.shape[0]
    rule = NB.bounded_rule(af_sim, peq, k, as_distance)
    want_nbr, want_val = NB.nearest_of_square(peq, k, as_distance)
    assert np.array_equal(rule["nbr"], want_nbr) and np.array_equal(rule["val"].view(np.uint64), want_val.view(np.uint64))
    kk = min(k, n - 1)
    assert len(rule["seed"][0]) <= n * kk and (rule["seed"][0] < rule["seed"][1]).all()
    # the bar is no better than the true kk-th best, and every true top-kk pair is a candidate
    worse = want_val[:, kk - 1] <= rule["bar"] if as_distance else want_val[:, kk - 1] >= rule["bar"]
    assert worse.all()
    listed = set(zip(rule["candidates"][0].tolist(), rule["candidates"][1].tolist()))
    assert all((min(g, h), max(g, h)) in listed for g in range(n) for h in want_nbr[g].tolist())
    if as_distance:
        assert rule["n_candidates"] >= PROPOSED[name][k]


def test_where_the_fallback_cap_lands():
    for as_distance in (True, False):
        af_sim, peq = squares("small", as_distance)
        assert NB.bounded_rule(af_sim, peq, 16, as_distance)["fallback"]
        af_sim, peq = squares("synth200", as_distance)
        for k in (1, 4, 16):
            rule = NB.bounded_rule(af_sim, peq, k, as_distance)
            assert not rule["fallback"] and 2 * rule["n_candidates"] <= 19900
    assert 2 * PROPOSED["small"][16] > 253 and 2 * PROPOSED["synth200"][16] <= 19900


def test_af_bound_command_line():
    from phamclust_amd import cli
    args = cli.parse_args(["in.tsv", "out", "-m", "peq", "--nearest", "5", "--af-bound"])
    assert args.af_bound and args.nearest == 5 and cli.DEFAULTS["af_bound"] is False and not cli.parse_args(["in.tsv", "out"]).af_bound
    assert cli.parse_args(["in.tsv", "out", "--nearest", "5", "--af-bound"]).af_bound               # (peq is the default metric)
    for bad in (["--af-bound"], ["--af-bound", "-m", "peq"], ["--af-bound", "--nearest", "5", "-m", "aai"], ["--af-bound", "--nearest", "5", "-m", "af"],
                ["--af-bound", "--nearest", "5", "-m", "jc"], ["--af-bound", "--nearest", "5", "-m", "peq", "--gpus", "2"],
                ["--af-bound", "--nearest", "5", "-m", "peq", "--grow-nearest", "old.tsv"], ["--af-bound", "--adjacency-only", "-m", "peq", "--edge-thresh", "0.5"],
                ["--af-bound", "--tree", "-m", "peq"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
    # --prefilter keeps its own refusals: it is no synonym
    with pytest.raises(SystemExit):
        cli.parse_args(["in.tsv", "out", "-m", "peq", "--nearest", "5", "--prefilter"])
    assert "--af-bound" in cli.build_parser().format_help()
    from phamclust_amd.scripts.phamclust import phamclust
    base = (None, None, False, "peq", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    with pytest.raises(ValueError, match="nearest_bound"):
        phamclust(*base, nearest_bound=True)
    with pytest.raises(ValueError, match="nearest_bound"):
        phamclust(*base, nearest_bound=True, nearest=3, grow_nearest="old.tsv")
    with pytest.raises(ValueError, match="nearest_bound"):
        phamclust(None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False, nearest_bound=True, nearest=3)


def test_bound_refuses_before_any_library_call(monkeypatch, small_genomes):
    from phamclust_amd import cli, hip, matrix as M

    def no_gpu(*args, **kwargs):
        raise AssertionError("a refusal must come before any GPU call")
    monkeypatch.setattr(hip.Context, "upload", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes._packed_of", no_gpu)
    monkeypatch.setattr(hip, "load", no_gpu)
    for metric in ("gcs", "jc", "pocp", "af", "aai"):
        with pytest.raises(ValueError, match="bound=True"):
            M.neighbors_de_novo(small_genomes, cli.METRICS[metric], 4, bound=True)
    with pytest.raises(ValueError, match="bound=True"):
        M.neighbors_de_novo(small_genomes, lambda s, t, as_distance=True: 0.0, 4, bound=True)
    with pytest.raises(ValueError, match="k must be"):
        M.neighbors_de_novo(small_genomes, cli.METRICS["peq"], 65, bound=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.neighbors_de_novo(small_genomes, cli.METRICS["peq"], 4, bound=True)


def test_the_header_and_the_binding(native_built):
    from phamclust_amd import hip
    from phamclust_amd.results import neighbors
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in hip.EXPORTS and hip.EXPORTS.count(name) == 1
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 172 and hip.load().pc_version() >= 172
    assert hasattr(hip.Context, "fill_edges_bars") and hasattr(hip.Context, "nearest_of_pairs") and not hasattr(hip.MultiContext, "nearest_of_pairs")
    assert hip.Context.NEAREST_PAIRS_MAX == neighbors.NEAREST_PAIRS_MAX == 2 ** 30
    assert neighbors.PREFILTER_SLACK == NB.PREFILTER_SLACK
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(REPO, doc)).read()
        assert all(name in text for name in NEW_EXPORTS), doc
