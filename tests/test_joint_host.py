"""The joint fill's host side, without a GPU: the exports, the metric-set helper, the refusals of ``matrices_de_novo`` and
``pairs_joint_de_novo`` that come before any GPU call, and the ``--also`` argument collisions."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

JOINT_SYMBOLS = ("pc_fill_joint", "pc_fill_joint_dev", "pc_fill_pairs_joint", "pc_fill_pairs_joint_dev")


def test_joint_fills_are_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    hooks_path = os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")
    for name in JOINT_SYMBOLS:
        assert re.search(r"\bint %s\s*\(pc_ctx\* ctx, uint32_t metrics, int as_distance," % name, header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, hooks_path):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
        assert getattr(hip.load(), name).argtypes[1] is ctypes.c_uint32
    assert int(re.search(r"#define PC_VERSION (\d+)", header).group(1)) >= 173
    assert hip.load().pc_version() >= 173 and ctypes.CDLL(hooks_path).pc_version() >= 173
    for method in ("fill_joint", "fill_joint_dev", "fill_pairs_joint", "fill_pairs_joint_dev"):
        assert hasattr(hip.Context, method), method
    from phamclust_amd import matrix, routes
    from phamclust_amd.results import pairs
    assert matrix.pairs_joint_de_novo is pairs.pairs_joint_de_novo and callable(matrix.matrices_de_novo)
    assert matrix._metric_names is routes._metric_names


def test_the_mask_helper():
    from phamclust_amd import hip
    assert hip.JOINT_METRICS == ("gcs", "jc", "pocp", "af", "aai", "peq")
    assert [hip.METRIC_IDS[name] for name in hip.JOINT_METRICS] == list(range(6))          # bit m of the mask is metric m of the enum
    assert hip.joint_mask(hip.JOINT_METRICS) == 0x3f
    assert hip.joint_mask(["peq"]) == hip.joint_mask("peq") == 1 << 5 and hip.joint_mask(("aai",)) == 1 << 4
    assert hip.joint_mask(["peq", "af"]) == hip.joint_mask(["af", "peq"]) == (1 << 3 | 1 << 5)
    assert hip.joint_mask(name for name in ("gcs", "aai")) == (1 | 1 << 4)
    with pytest.raises(ValueError, match="empty"):
        hip.joint_mask([])
    with pytest.raises(ValueError, match="unknown"):
        hip.joint_mask(["peq", "ani"])
    with pytest.raises(ValueError, match="unknown"):
        hip.joint_mask(["aai_ppos", "peq"])                        # another alignment pass: no part of a joint fill
    with pytest.raises(ValueError, match="twice"):
        hip.joint_mask(["peq", "af", "peq"])
    for alone in (["gcs"], ["af"], ["gcs", "jc", "pocp", "af"]):
        with pytest.raises(ValueError, match="neither aai nor peq"):
            hip.joint_mask(alone)
    out = hip.Context._joint_pointers(1 << 3 | 1 << 5, lambda name: {"af": 24, "peq": 40}[name])
    assert [out[m] for m in range(6)] == [None, None, None, 24, None, 40]


def test_joint_routes_refuse_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import cli, hip, matrix as M
    names = [g.name for g in small_genomes]
    peq, af = cli.METRICS["peq"], cli.METRICS["af"]

    def no_gpu(*args, **kwargs):
        raise AssertionError("a refusal must come before any GPU call")
    monkeypatch.setattr(hip.Context, "upload", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes.get_context", no_gpu)
    monkeypatch.setattr("phamclust_amd.routes._packed_of", no_gpu)
    stranger = lambda s, t, as_distance=True: 0.0                  # noqa: E731
    for call in (lambda funcs: M.matrices_de_novo(small_genomes, funcs, 1), lambda funcs: M.pairs_joint_de_novo(small_genomes, funcs, [(0, 1)])):
        with pytest.raises(ValueError, match="empty"):
            call([])
        with pytest.raises(ValueError, match=r"funcs\[1\] is none of the six METRICS"):
            call([peq, stranger])
        with pytest.raises(ValueError, match="'af' is listed twice"):
            call([af, peq, af])
        with pytest.raises(ValueError, match="'peq' is listed twice"):
            call(func for func in (peq, peq))
    assert M._metric_names([af, peq], "x") == ["af", "peq"] and M._metric_names(list(cli.METRICS.values()), "x") == list(cli.METRICS)
    with pytest.raises(ValueError, match="at least 1 genome"):
        M.matrices_de_novo([], [peq], 1)
    # pairs_de_novo's own refusals, in its order: the list is checked before the callables
    with pytest.raises(KeyError, match="no such genome"):
        M.pairs_joint_de_novo(small_genomes, [peq], [(names[0], "no such genome")])
    with pytest.raises(IndexError):
        M.pairs_joint_de_novo(small_genomes, [peq, af], np.array([[0, 1], [-1, 2]]))
    with pytest.raises(ValueError, match="no pair"):
        M.pairs_joint_de_novo(small_genomes, [peq], [(0, 1, 2)])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.matrices_de_novo(small_genomes, [peq, af], 1)
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.pairs_joint_de_novo(small_genomes, [peq, af], [(0, 1)])


def test_also_command_line(monkeypatch, capsys):
    from phamclust_amd import cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cli.DEFAULTS["also"] is None and cli.parse_args(["in.tsv", "out"]).also is None
    assert cli.parse_args(["in.tsv", "out", "-m", "peq", "--also", "af,aai"]).also == ["af", "aai"]
    assert cli.parse_args(["in.tsv", "out", "--also", "jc"]).also == ["jc"]                 # (-m's default is peq)
    assert cli.parse_args(["in.tsv", "out", "-m", "jc", "--also", "gcs, af", "--pairs", "edges.tsv"]).also == ["gcs", "af"]
    assert cli.parse_args(["in.tsv", "out", "-m", "aai", "-O", "peq", "--cluster-table", "--cluster-fit", "--distribution"]).also == ["peq"]
    assert "--also" in cli.build_parser().format_help()

    def refused(argv, *words):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + argv)
        message = capsys.readouterr().err
        for word in words:
            assert word in message, (argv, word, message)
    # the flags --also collides with, each named in the message
    for other, flag in ((["--gpus", "2"], "--gpus"), (["--extend", "old.tsv"], "--extend"), (["--no-matrix"], "--no-matrix"),
                        (["--adjacency-only"], "--adjacency-only"), (["--components-only"], "--components-only"), (["--nearest", "3"], "--nearest"),
                        (["--tree"], "--tree"), (["--distribution-only"], "--distribution-only"), (["--place", "fit.tsv"], "--place"),
                        (["--adjacency-only", "--edge-thresh", "0.5", "--prefilter"], "--adjacency-only"), (["--nearest", "3", "--af-bound"], "--nearest"),
                        (["--tree", "--grow", "tree_peq.tsv"], "--tree"), (["--nearest", "3", "--grow-nearest", "nearest_peq.tsv"], "--nearest")):
        refused(["-m", "peq", "--also", "af"] + other, "--also", flag)
    refused(["--pairs", "edges.tsv", "--also", "af", "--gpus", "2"], "--gpus")
    monkeypatch.setenv("WORLD_SIZE", "2")                                                   # a launcher job
    refused(["-m", "peq", "--also", "af"], "--also", "launcher")
    monkeypatch.delenv("WORLD_SIZE")
    # what it names
    refused(["-m", "peq", "--also", "peq"], "--also", "-m's own")
    refused(["--also", "af,peq"], "--also", "-m's own")
    refused(["-m", "peq", "--also", "af,ani"], "--also", "'ani'")
    refused(["-m", "peq", "--also", "aai_ppos"], "--also", "'aai_ppos'")
    refused(["-m", "peq", "--also", "af,aai,af"], "--also", "'af' is listed twice")
    refused(["-m", "peq", "--also", ""], "--also")
    # the same collisions for a library caller of phamclust()
    from phamclust_amd.scripts.phamclust import phamclust
    base = (None, None, False, "peq", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    for other in (dict(adjacency_only=True), dict(components_only=True), dict(no_matrix=True), dict(tree=True), dict(nearest=3), dict(extend="old.tsv"),
                  dict(distribution_only=True), dict(place="fit.tsv")):
        with pytest.raises(ValueError, match="also"):
            phamclust(*base, also=["af"], **other)
    for bad in (["peq"], ["af", "af"], ["ani"]):
        with pytest.raises(ValueError, match="also"):
            phamclust(*base, also=bad)
