"""Growing stored k-nearest lists on the host (no GPU): the binding of pc_fill_rows_nearest, ``NearestNeighbors.extended`` against
``from_dense`` of the grown matrix -- the proof the feature rests on, run where it can be run -- the refusals of ``neighbors_extend`` and
of --grow-nearest, the guard, and the file's round trip.  Everything is exact."""

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden_file, read_lower_triangle

NEW_EXPORTS = ("pc_fill_rows_nearest", "pc_nearest_rows_tile")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def dense(names, square, is_distance):
    from phamclust_amd.matrix import _square_matrix
    return _square_matrix(names, np.array(square, dtype=np.float64), is_distance)


def golden_square(metric):
    names, condensed, _ = read_lower_triangle(golden_file(metric))
    n = len(names)
    square = np.zeros((n, n))
    square[np.triu_indices(n, k=1)] = condensed
    return names, square + square.T


# ---- binding ------------------------------------------------------------------------------------------------------
def test_rows_nearest_is_exported_everywhere(native_built):
    from phamclust_amd import hip
    header = open(os.path.join(REPO, "include", "phamclust_hip.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        for lib in (hip.LIB_PATH, os.path.join(os.path.dirname(hip.LIB_PATH), "libphamclust_hip_hooks.so")):
            assert hasattr(ctypes.CDLL(lib), name), (lib, name)
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) >= 163 and hip.load().pc_version() >= 163
    assert hasattr(hip.Context, "fill_rows_nearest") and not hasattr(hip.MultiContext, "fill_rows_nearest")      # a one-GPU call
    assert hip.Context.nearest_rows_tile() == 64
    assert hip.Context.ROWS_PASSES == ("edges", "components", "tree") and hip.load().pc_rows_pass_span(3) == 0     # no fourth flat pass


def test_library_refuses_before_upload(native_built):
    """No context: PC_ERR_STATE, every output nulled, before anything touches a device."""
    from phamclust_amd import hip
    lib = hip.load()
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    junk_i, junk_d = (ctypes.c_int32 * 1)(1), (ctypes.c_double * 1)(1.0)
    pn, pv = ctypes.cast(junk_i, i32p), ctypes.cast(junk_d, f64p)
    kk, nsl = ctypes.c_int32(5), ctypes.c_int32(5)
    rows = (ctypes.c_int32 * 1)(0)
    rc = lib.pc_fill_rows_nearest(None, 1, 1, 3, rows, 1, None, None, 0, 0, ctypes.byref(pn), ctypes.byref(pv), ctypes.byref(kk), ctypes.byref(nsl), None)
    assert rc != 0 and b"pc_fill_rows_nearest: upload first" in lib.pc_last_error()
    assert not pn and not pv and kk.value == 0 and nsl.value == 0


# ---- the proof: extended() of the old block is from_dense() of the grown matrix -------------------------------------
def tied_matrix(rng, n, twins):
    """A symmetric matrix of millionths drawn from at most 8 levels, with ``twins`` pairs of identical rows."""
    levels = np.sort(rng.choice(1000001, size=int(rng.integers(1, 9)), replace=False)) / 1000000.0
    square = levels[rng.integers(0, levels.shape[0], size=(n, n))]
    square = np.triu(square, 1)
    square = square + square.T
    for _ in range(twins):
        a, b = rng.choice(n, size=2, replace=False).tolist()
        square[b, :], square[:, b] = square[a, :], square[:, a]
        square[a, b] = square[b, a] = levels[0]
    return square


def splits(rng, n):
    """New sets of n nodes: one new (first, last, inside), one old, all new, adjacent runs and scattered sets of every other size class."""
    out = [[0], [n - 1], [n // 2], list(range(n)), [g for g in range(n) if g != int(rng.integers(0, n))]]
    for size in sorted({2, n // 2, n - 2} & set(range(1, n))):
        a = int(rng.integers(0, n - size + 1))
        out.append(list(range(a, a + size)))
        out.append(sorted(rng.choice(n, size=size, replace=False).tolist()))
    seen, unique = set(), []
    for new in out:
        if tuple(new) not in seen:
            seen.add(tuple(new))
            unique.append(new)
    return unique


@pytest.mark.parametrize("is_distance", [True, False])
def test_extended_equals_from_dense_of_the_grown_matrix(is_distance):
    from phamclust_amd.matrix import NearestNeighbors
    rng = np.random.default_rng(11 + is_distance)
    short = complete = 0
    for n in range(2, 41):
        square = tied_matrix(rng, n, twins=int(n > 3) * int(rng.integers(0, 3)))
        np.fill_diagonal(square, 0.0 if is_distance else 1.0)
        names = [f"g{g:03d}" for g in range(n)]
        whole = dense(names, square, is_distance)
        for new in splits(rng, n):
            old = [g for g in range(n) if g not in set(new)]
            for k in sorted({1, 2, int(rng.integers(1, n + 2)), n - 1, 64}):
                label = (is_distance, n, new, k)
                if old:
                    stored = NearestNeighbors.from_dense(dense([names[g] for g in old], square[np.ix_(old, old)], is_distance), k)
                else:
                    stored = NearestNeighbors([], np.empty((0, 0)), np.empty((0, 0)), is_distance=is_distance)
                short += len(old) - 1 < k
                complete += bool(old) and stored.k == k
                got, want = stored.extended(names, new, square[new], k=k), NearestNeighbors.from_dense(whole, k)
                assert got.nodes == want.nodes and got.is_distance == is_distance and got.k == want.k == min(k, n - 1), label
                assert got.indices.dtype == np.int32 and np.array_equal(got.indices, want.indices), label
                assert same_bits(got.weights, want.weights), label
                if stored.k == k:                                            # k defaults to the stored k
                    again = stored.extended(names, new, square[new])
                    assert np.array_equal(again.indices, want.indices) and same_bits(again.weights, want.weights), label
    assert short and complete


def test_extended_refuses_what_cannot_be_grown():
    from phamclust_amd.matrix import NearestNeighbors
    stored = NearestNeighbors(["a", "c", "d"], [[1], [0], [0]], [[0.5], [0.5], [0.6]])
    rows = np.array([[0.25, 0.0, 0.75, 0.1]])
    grown = stored.extended(["a", "b", "c", "d"], [1], rows)
    assert list(grown) == [("a", "b", 0.25), ("b", "d", 0.1), ("c", "a", 0.5), ("d", "b", 0.1)]
    with pytest.raises(ValueError, match="cannot decide 2"):                 # one of two old neighbours stored: the second is unknown
        stored.extended(["a", "b", "c", "d"], [1], rows, k=2)
    with pytest.raises(ValueError, match="another order"):
        stored.extended(["d", "c", "b", "a"], [2], rows)
    with pytest.raises(KeyError, match="'c'"):
        stored.extended(["a", "b", "d", "e"], [1, 3], np.zeros((2, 4)))
    with pytest.raises(ValueError, match="distinct"):
        stored.extended(["a", "b", "b", "c", "d"], [1, 2], np.zeros((2, 5)))
    with pytest.raises(ValueError, match="exactly the nodes that are not stored"):
        stored.extended(["a", "b", "c", "d"], [0, 1], np.zeros((2, 4)))
    with pytest.raises(TypeError):
        stored.extended(["a", "b", "c", "d"], [1], np.array([[0.25, 0.0, np.nan, 0.1]]))


def test_without_raises():
    from phamclust_amd.matrix import NearestNeighbors
    stored = NearestNeighbors(["a", "c"], [[1], [0]], [[0.5], [0.5]])
    with pytest.raises(ValueError, match="only a fill knows"):
        stored.without(["a"])
    with pytest.raises(ValueError):
        stored.without([])


# ---- the call's refusals, all before a GPU call ---------------------------------------------------------------------
def _stored(small_genomes, drop, k=5):
    from phamclust_amd.matrix import NearestNeighbors
    names, square = golden_square("jc")
    assert names == [g.name for g in small_genomes]
    keep = [g for g in range(len(names)) if g not in drop]
    return NearestNeighbors.from_dense(dense([names[g] for g in keep], square[np.ix_(keep, keep)], True), k), names, square


def test_neighbors_extend_refuses_before_any_gpu_call(monkeypatch, small_genomes):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    jc = cli.METRICS["jc"]
    stored, _, _ = _stored(small_genomes, {3, 4})
    other = lambda s, t, as_distance=True: 0.0                                # noqa: E731
    with pytest.raises(ValueError, match="no CPU route"):
        M.neighbors_extend(stored, small_genomes, other)
    with pytest.raises(ValueError):
        M.neighbors_extend(stored, [], jc)
    with pytest.raises(KeyError, match="is not among the genomes"):
        M.neighbors_extend(stored, small_genomes[1:], jc)                    # stored node 0 is no genome
    with pytest.raises(ValueError, match="another order"):
        M.neighbors_extend(stored, small_genomes[::-1], jc)
    with pytest.raises(ValueError, match="distinct"):
        M.neighbors_extend(stored, small_genomes + small_genomes[:1], jc)
    with pytest.raises(ValueError, match="cannot decide 6"):
        M.neighbors_extend(stored, small_genomes, jc, k=6)
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="k must be an integer"):
            M.neighbors_extend(stored, small_genomes, jc, k=bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one-GPU"):
        M.neighbors_extend(stored, small_genomes, jc)


def test_nothing_new_returns_the_stored_lists_relaid(small_genomes):
    """No new genome: no fill, no GPU -- the stored lists on the genomes' names, cut after k."""
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    jc = cli.METRICS["jc"]
    stored, names, _ = _stored(small_genomes, set())
    got = M.neighbors_extend(stored, small_genomes, jc)
    assert got.nodes == names and np.array_equal(got.indices, stored.indices) and same_bits(got.weights, stored.weights)
    got = M.neighbors_extend(stored, small_genomes, jc, k=2)
    assert got.k == 2 and np.array_equal(got.indices, stored.indices[:, :2]) and same_bits(got.weights, stored.weights[:, :2])
    full, _, _ = _stored(small_genomes, set(), k=64)                        # complete lists: a larger k is no refusal
    assert M.neighbors_extend(full, small_genomes, jc, k=64).k == len(names) - 1


# ---- the guard (host route: the check the call makes, on refilled rows computed here) ------------------------------------
def test_guard_raises_on_the_verified_rows(small_genomes):
    from phamclust_amd import matrix as M
    stored, names, square = _stored(small_genomes, {3, 4})
    old_at = np.asarray([g for g in range(len(names)) if g not in (3, 4)], dtype=np.int64)
    checked = [int(g) for g in old_at]                                        # every old genome verified
    values = square[checked]
    indices = old_at[stored.indices]
    M._guard_neighbors(names, "jc", checked, values, old_at, indices, stored.weights, True)          # the true lists pass
    off = stored.weights.copy()
    off[7, 2] = round(off[7, 2] + 1e-6, 6)                                    # a stored value off by one millionth
    with pytest.raises(ValueError, match=r"pair \(\S+, \S+\): the nearest-neighbours list holds"):
        M._guard_neighbors(names, "jc", checked, values, old_at, indices, off, True)
    _, other_square = golden_square("gcs")                                    # another metric's rows
    with pytest.raises(ValueError, match="was not filled with this metric"):
        M._guard_neighbors(names, "jc", checked, other_square[checked], old_at, indices, stored.weights, True)
    swapped = old_at.copy()                                                   # a permuted node order: the stored indices name other genomes
    swapped[[0, 1]] = swapped[[1, 0]]
    with pytest.raises(ValueError, match="the nearest-neighbours list holds"):
        M._guard_neighbors(names, "jc", checked, values, old_at, swapped[stored.indices], stored.weights, True)
    M._guard_neighbors(names, "jc", [], values[:0], old_at, indices, off, True)                      # verify=0: no check


# ---- the file -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_file_round_trip_bit_for_bit(metric, tmp_path):
    from phamclust_amd import matrix as M
    names, condensed, _ = read_lower_triangle(golden_file(metric))
    whole = M.SymMatrix.from_condensed(names, condensed, is_distance=True)
    for k in (1, 5, 64):
        found = M.NearestNeighbors.from_dense(whole, k)
        path = M.nearest_to_file(found, tmp_path / f"nearest_{metric}.tsv")
        assert open(path).read() == "".join(f"{s}\t{t}\t{w:.6f}\n" for s, t, w in found.inverted())     # the bytes --nearest has always written
        back = M.nearest_from_file(path, names)
        assert back.nodes == found.nodes and back.is_distance and back.k == found.k
        assert np.array_equal(back.indices, found.indices) and same_bits(back.weights, found.weights)
        sub = M.nearest_from_file(path, ["!before"] + names + ["~after"])     # a longer genome list: the file's sources only
        assert sub.nodes == found.nodes and np.array_equal(sub.indices, found.indices)
    lines = open(path).read().splitlines(keepends=True)
    per = len(names) - 1

    def refused(text, error, match):
        bad = tmp_path / "bad.tsv"
        bad.write_text(text)
        with pytest.raises(error, match=match):
            M.nearest_from_file(bad, names)

    with pytest.raises(KeyError, match="is not among the genomes"):
        M.nearest_from_file(path, names[1:])
    refused("".join(lines[:-1]) + "a\tb\n", ValueError, "expected source<TAB>target<TAB>similarity")
    refused("".join(lines[:-1]) + lines[-1].replace("\n", "\textra\n"), ValueError, "expected source<TAB>target<TAB>similarity")
    refused("".join(lines[:-1]) + "\t".join(lines[-1].split("\t")[:2]) + "\tnear\n", ValueError, "is no similarity")
    refused("".join(lines[:-1]) + "\t".join(lines[-1].split("\t")[:2]) + "\t1.5\n", ValueError, r"outside \[0, 1\]")
    refused("".join(lines[:-1]), ValueError, "every source lists the same number")                    # unequal lines per source
    refused("".join(lines[per:2 * per] + lines[:per] + lines[2 * per:]), ValueError, "another order")
    refused("".join(lines) + lines[0], ValueError, "another order")                                   # a source's lines not together
    small = M.NearestNeighbors.from_dense(M.SymMatrix.from_condensed(names[:3], condensed[[0, 1, len(names) - 1]], is_distance=True), 2)
    text = open(M.nearest_to_file(small, tmp_path / "small.tsv")).read().splitlines(keepends=True)
    refused("".join(line for pair in zip(text[0::2], text[1::2], text[0::2]) for line in pair), ValueError, r"is no min\(K, n - 1\)")
    for stranger in (names[5], names[1], names[2]):                          # no source of the file, the source itself, listed twice
        refused("".join(text[:2]) + "".join(text[2:4]).replace(f"\t{names[0]}\t", f"\t{stranger}\t") + "".join(text[4:]), ValueError, "distinct other sources")
    assert len(M.nearest_from_file(tmp_path / "small.tsv", names).nodes) == 3


# ---- the command line ---------------------------------------------------------------------------------------------
def test_grow_nearest_command_line(capsys):
    from phamclust_amd import cli
    from phamclust_amd.scripts import phamclust as script
    args = cli.parse_args(["in.tsv", "out", "-m", "jc", "--nearest", "5", "--grow-nearest", "nearest_jc.tsv"])
    assert args.nearest == 5 and str(args.grow_nearest) == "nearest_jc.tsv" and cli.DEFAULTS["grow_nearest"] is None
    assert cli.parse_args(["in.tsv", "out", "--nearest", "5"]).grow_nearest is None
    for bad in (["--grow-nearest", "f"], ["--grow-nearest", "f", "--tree"], ["--grow-nearest", "f", "--nearest", "5", "--gpus", "2"],
                ["--grow-nearest", "f", "--nearest", "5", "--adjacency-only"], ["--grow-nearest", "f", "--nearest", "5", "--components-only"],
                ["--grow-nearest", "f", "--nearest", "5", "--no-matrix"], ["--grow-nearest", "f", "--nearest", "5", "--extend", "old.tsv"],
                ["--grow-nearest", "f", "--nearest", "5", "--tree"], ["--grow-nearest", "f", "--nearest", "5", "--grow", "g"],
                ["--grow-nearest", "f", "--nearest", "65"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["in.tsv", "out"] + bad)
        err = capsys.readouterr().err
        assert "--grow-nearest" in err or "--nearest" in err or "--grow" in err, bad
    with pytest.raises(SystemExit):                                          # the older refusal stands: --grow has no nearest route
        cli.parse_args(["in.tsv", "out", "--grow", "f", "--nearest", "3"])
    assert "--grow FILE grows a stored tree (--tree) or stored components" in capsys.readouterr().err
    plan = script.gpus_plan(cli.parse_args(["in.tsv", "out", "--nearest", "5", "--grow-nearest", "f"]), "process", None)
    assert plan[:2] == (1, "one") and "one-GPU call" in plan[2] and "--grow-nearest" in plan[2]
    assert "--grow-nearest" in cli.build_parser().format_help()


def test_phamclust_checks_grow_nearest_before_any_gpu_call(monkeypatch):
    """The argument checks of phamclust(..., grow_nearest=...) come first: nothing is read, logged or uploaded."""
    import inspect
    from phamclust_amd import matrix as M
    from phamclust_amd.scripts import phamclust as script

    def reached(*args, **kwargs):
        raise AssertionError("a refusal came after the run had begun")

    monkeypatch.setattr(script, "_Run", reached)
    monkeypatch.setattr("phamclust_amd.routes.upload_for_fills", reached)
    assert list(inspect.signature(script.phamclust).parameters)[-2:] == ["grow_nearest", "nearest"]     # (an older test pins nearest as the last one)
    assert inspect.signature(script.phamclust).parameters["grow_nearest"].default is None
    base = (None, None, False, "jc", 0.0, "complete", 0.5, "average", 0.3, "single", 1, False, None, 0.5, 1, False, False)
    for other in (dict(), dict(tree=True), dict(nearest=5, grow="g"), dict(nearest=5, adjacency_only=True), dict(nearest=5, components_only=True),
                  dict(nearest=5, no_matrix=True), dict(nearest=5, extend="old.tsv"), dict(nearest=5, tree=True), dict(nearest=65), dict(nearest=True)):
        with pytest.raises(ValueError):
            script.phamclust(*base, grow_nearest="f", **other)
