"""The host side of the edge, component and nearest fills over several GPUs (no GPU): ``pc_stretch_plan`` -- the deal of contiguous
stretches of target genomes, one per device -- against a pure-Python restatement of its definition and the properties that follow
from it, its refusals, the new exports in header, libraries and binding, and what ``--adjacency-only`` / ``--components-only`` /
``--nearest`` come to with ``--gpus N`` (the parser and ``gpus_plan``, the route decision of the command line)."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW_EXPORTS = ("pc_multi_fill_edges", "pc_multi_fill_components", "pc_multi_fill_nearest", "pc_multi_last_stretches",
               "pc_multi_last_slab_times", "pc_stretch_plan")


def stretch_plan(cost, world):
    """The definition, in Python integers: bounds[r] = the smallest t in [0, n] with P(t) * world >= r * P(n)."""
    cost = [int(c) for c in cost]
    n = len(cost)
    prefix = [0]
    for c in cost:
        prefix.append(prefix[-1] + c)
    bounds = [0]
    for r in range(1, world):
        bounds.append(next(t for t in range(n + 1) if prefix[t] * world >= r * prefix[n]))
    return bounds + [n]


def cost_vectors():
    rng = np.random.default_rng(20260)
    out = {"empty": [], "one": [7], "one zero": [0], "two": [0, 1], "two equal": [5, 5], "zeros": [0] * 9,
           "ramp": list(range(40)), "ramp 3": [0, 1, 2],
           "single huge": [3, 1, 4, 2 ** 62, 1, 5, 9, 2], "huge first": [2 ** 62, 1, 1, 1], "huge last": [1, 1, 1, 2 ** 62],
           "near 2^63": [2 ** 61] * 3 + [2 ** 60, 2 ** 59, 12345],
           "aligned": [2000 * t + int(x) for t, x in enumerate(rng.integers(0, 10 ** 9, 200))]}
    for k in range(12):
        n = int(rng.integers(1, 90))
        values = rng.integers(0, 10 ** int(rng.integers(1, 15)), n)
        values[rng.random(n) < 0.3] = 0                                    # zeros among them: empty stretches, repeated bounds
        out[f"random {k}"] = values.tolist()
    return out


COSTS = cost_vectors()


@pytest.mark.parametrize("name", sorted(COSTS))
def test_stretch_plan_equals_its_definition(native_built, name):
    from phamclust_amd.hip import MultiContext
    cost = COSTS[name]
    n, total = len(cost), sum(cost)
    assert total < 2 ** 63
    for world in range(1, 10):                                             # 1..9: above n for the short vectors
        bounds = MultiContext.slab_stretches(cost, world)
        label = (name, world)
        assert bounds.dtype == np.int32 and bounds.shape == (world + 1,), label
        got = bounds.tolist()
        assert got == stretch_plan(cost, world), label
        assert got[0] == 0 and got[-1] == n, label
        assert all(a <= b for a, b in zip(got, got[1:])), label            # monotone; a stretch may be empty
        for a, b in zip(got, got[1:]):                                     # no stretch above its share by more than its last target
            if b > a:
                assert sum(cost[a:b]) * world <= total + cost[b - 1] * world, label
        if world == 1:
            assert got == [0, n], label
    if name == "ramp 3":                                                   # three genomes on four devices: what the GPU tests meet
        assert MultiContext.slab_stretches(cost, 4).tolist() == [0, 2, 3, 3, 3]
    if name == "two":
        assert MultiContext.slab_stretches(cost, 4).tolist() == [0, 2, 2, 2, 2]
    if name == "zeros":
        assert MultiContext.slab_stretches(cost, 3).tolist() == [0, 0, 0, 9]


def test_stretch_plan_refusals(native_built):
    from phamclust_amd import hip
    lib = hip.load()
    cost = np.arange(5, dtype=np.uint64)
    bounds = np.full(8, -7, dtype=np.int32)
    u64p, i32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)
    c, b = cost.ctypes.data_as(u64p), bounds.ctypes.data_as(i32p)
    assert lib.pc_stretch_plan(c, -1, 2, b) == -1 and b"pc_stretch_plan" in lib.pc_last_error()
    assert lib.pc_stretch_plan(c, 5, 0, b) == -1 and lib.pc_stretch_plan(c, 5, -3, b) == -1
    assert lib.pc_stretch_plan(None, 5, 2, b) == -1 and lib.pc_stretch_plan(c, 5, 2, None) == -1
    assert (bounds == -7).all()                                            # a refusal writes nothing
    assert lib.pc_stretch_plan(c, 0, 3, b) == 0 and bounds[:4].tolist() == [0, 0, 0, 0] and bounds[4] == -7
    assert lib.pc_stretch_plan(c, 5, 2, b) == 0 and bounds[:3].tolist() == [0, 4, 5]      # P = 0 0 1 3 6 10: 2 P(4) = 12 >= 10
    with pytest.raises(hip.HipLibraryError):
        hip.MultiContext.slab_stretches(cost, 0)


def test_new_calls_are_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 160
    assert hip.load().pc_version() >= 160
    for method in ("fill_edges", "fill_components", "fill_nearest", "slab_stretches"):
        assert hasattr(hip.MultiContext, method), method
    # the multi calls take their single-context namesakes' arguments, with the pc_multi handle in the context's place
    lib = hip.load()
    for name in ("edges", "components", "nearest"):
        assert getattr(lib, f"pc_multi_fill_{name}").argtypes == getattr(lib, f"pc_fill_{name}").argtypes
    import inspect
    for name in ("fill_edges", "fill_components", "fill_nearest"):
        assert inspect.signature(getattr(hip.MultiContext, name)) == inspect.signature(getattr(hip.Context, name)), name


# ---- command line ---------------------------------------------------------------------------------------
FLAGS = (["--adjacency-only"], ["--components-only"], ["--nearest", "5"])


def test_the_three_flags_parse_with_gpus():
    from phamclust_amd import cli
    for flag in FLAGS:
        args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--gpus", "4"] + flag)
        assert args.gpus == 4 and (args.adjacency_only or args.components_only or args.nearest == 5)
    with pytest.raises(SystemExit):                                        # --no-matrix keeps refusing --gpus
        cli.parse_args(["in.tsv", "out", "--no-matrix", "--gpus", "2"])
    text = cli.build_parser().format_help()
    assert text.count("spread over N GPUs of this process") == 3


def test_route_decisions_of_the_three_flags(native_built, monkeypatch):
    from phamclust_amd import cli
    from phamclust_amd.scripts.phamclust import gpus_plan
    from phamclust_amd.synth import synth_packed
    for key in ("PHAMCLUST_FORCE_GPUS", "PHAMCLUST_LAUNCH_COST_S", "PHAMCLUST_MULTI"):
        monkeypatch.delenv(key, raising=False)
    small = synth_packed(120, 1500, seed=4)
    for flag in FLAGS:
        args = cli.parse_args(["in.tsv", "out", "-m", "peq", "--gpus", "2"] + flag)
        # in this process: the dense fill's estimate decides, and without one (a genome directory) the request stands
        assert gpus_plan(args, "process", None) == (2, "process", None)
        n, how, note = gpus_plan(args, "process", small)                   # 120 genomes: milliseconds of fill, not worth a second device
        assert (n, how) == (1, "one") and "running on ONE GPU" in note and "a context and an upload per device" in note
        monkeypatch.setenv("PHAMCLUST_FORCE_GPUS", "1")
        n, how, note = gpus_plan(args, "process", small)
        assert (n, how) == (2, "process") and "PHAMCLUST_FORCE_GPUS" in note
        # one process per GPU has no route for them: today's note, whatever the estimate would say
        n, how, note = gpus_plan(args, "launcher", small)
        assert (n, how) == (1, "one") and "is a one-GPU call: the matrix stage stays on one GPU" in note and flag[0] in note
        monkeypatch.delenv("PHAMCLUST_FORCE_GPUS")
    # the dense fill and --extend decide as before
    dense = cli.parse_args(["in.tsv", "out", "-m", "peq", "--gpus", "2"])
    assert gpus_plan(dense, "launcher", None) == (2, "launcher", None) and gpus_plan(dense, "process", None) == (2, "process", None)
    assert gpus_plan(dense, "process", small)[:2] == (1, "one")
    extend = cli.parse_args(["in.tsv", "out", "-m", "jc", "--gpus", "2", "--extend", "old.tsv"])
    for route in ("process", "launcher"):
        n, how, note = gpus_plan(extend, route, None)
        assert (n, how) == (1, "one") and "--extend" in note and "one-GPU call" in note
    device = cli.parse_args(["in.tsv", "out", "-m", "jc", "--gpus", "2", "--device", "1", "--nearest", "5"])
    assert "--device 1 is IGNORED" in gpus_plan(device, "process", None)[2]


def test_de_novo_calls_choose_the_multi_context(monkeypatch):
    """``PHAMCLUST_GPU_IDS`` / ``PHAMCLUST_GPUS`` naming several devices: the three calls take the MultiContext; one device, or none
    named: the one-GPU context; under a launcher they raise as before (tests/test_edges_host.py and its siblings pin the message)."""
    from phamclust_amd import matrix as M
    made = []
    monkeypatch.setattr("phamclust_amd.routes.get_multi_context", lambda ids: made.append(("multi", list(ids))) or "multi")
    monkeypatch.setattr("phamclust_amd.routes.get_context", lambda device=None: made.append(("one", device)) or "one")
    for key in ("WORLD_SIZE", "PHAMCLUST_GPUS", "PHAMCLUST_GPU_IDS"):
        monkeypatch.delenv(key, raising=False)
    assert M._slab_fill_context() == ("one", 1)
    monkeypatch.setenv("PHAMCLUST_GPUS", "3")
    assert M._slab_fill_context() == ("multi", 3)
    monkeypatch.setenv("PHAMCLUST_GPU_IDS", "0,0")
    assert M._slab_fill_context() == ("multi", 2)
    monkeypatch.setenv("PHAMCLUST_GPU_IDS", "2")
    assert M._slab_fill_context() == ("one", 1)
    monkeypatch.setenv("WORLD_SIZE", "2")                                  # a launcher: in_process_devices() answers None
    assert M._slab_fill_context() == ("one", 1)
    assert made == [("one", None), ("multi", [0, 1, 2]), ("multi", [0, 0]), ("one", 2), ("one", None)]
