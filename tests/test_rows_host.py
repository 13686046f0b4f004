"""matrix_extend and the --extend flag on the host (no GPU): the generic per-pair path over the new pairs only, and the
corner cases of the container work.  The GPU half is tests/test_gpu_rows.py."""

import numpy as np
import pytest

from phamclust_amd.matrix import SymMatrix, matrix_de_novo, matrix_extend


def _toy_directed(source, target, as_distance=False):
    """None of the six METRICS, and NOT symmetric in (source, target): the generic path must keep matrix_de_novo's orientation
    (source = the earlier genome of the list).  Module level: joblib pickles it by name."""
    union = len(source | target)
    sim = (len(source & target) + 0.25 * (len(source) > len(target))) / (union + 1) if union else 0.0
    return round(1.0 - sim, 6) if as_distance else round(sim, 6)


def _subsets(n):
    return {"interleaved": [k for k in range(n) if k % 3 != 1], "prefix": list(range(n - 5)), "suffix": list(range(4, n)),
            "one old": [n // 2], "one new": [k for k in range(n) if k != 7]}


@pytest.mark.parametrize("which", ["interleaved", "prefix", "suffix", "one old", "one new"])
@pytest.mark.parametrize("as_distance", [True, False])
def test_generic_extend_equals_de_novo(small_genomes, which, as_distance):
    """A callable outside METRICS: old block copied, new pairs computed per pair on the host -- the matrix of a whole fill."""
    whole = matrix_de_novo(small_genomes, _toy_directed, 1, as_distance=as_distance)
    keep = _subsets(len(small_genomes))[which]
    old = matrix_de_novo([small_genomes[k] for k in keep], _toy_directed, 1, as_distance=as_distance)
    got = matrix_extend(old, small_genomes, _toy_directed, 1)
    assert got.nodes == whole.nodes and got.is_distance == as_distance
    assert np.array_equal(got.to_ndarray(), whole.to_ndarray())
    # the old matrix in another node order gives the same: the result is laid out by `genomes`
    shuffled = old.extract_submatrix(old.nodes[::-1])
    assert np.array_equal(matrix_extend(shuffled, small_genomes, _toy_directed, 1).to_ndarray(), whole.to_ndarray())


def test_generic_extend_over_workers(small_genomes):
    whole = matrix_de_novo(small_genomes, _toy_directed, 1)
    old = whole.extract_submatrix([g.name for g in small_genomes[::2]])
    got = matrix_extend(old, small_genomes, _toy_directed, 2)
    assert np.array_equal(got.to_ndarray(), whole.to_ndarray())


def test_extend_corner_cases(small_genomes):
    names = [g.name for g in small_genomes]
    whole = matrix_de_novo(small_genomes, _toy_directed, 1)
    # nothing new: the matrix re-laid in `genomes` order (a new object; no metric call at all)
    def never(source, target, as_distance=False):
        raise AssertionError("nothing new: no pair may be computed")
    back = matrix_extend(whole.extract_submatrix(names[::-1]), small_genomes, never, 1)
    assert back.nodes == names and np.array_equal(back.to_ndarray(), whole.to_ndarray()) and back is not whole
    # every genome new: matrix_de_novo, of the old matrix's kind
    for kind in (True, False):
        fresh = matrix_extend(SymMatrix([], is_distance=kind), small_genomes, _toy_directed, 1)
        assert fresh.is_distance == kind
        assert np.array_equal(fresh.to_ndarray(), matrix_de_novo(small_genomes, _toy_directed, 1, as_distance=kind).to_ndarray())
    # an unset cell
    holed = whole.extract_submatrix(names[:10])
    holed._data[2, 5] = holed._data[5, 2] = np.nan
    with pytest.raises(ValueError, match="unset cell"):
        matrix_extend(holed, small_genomes, _toy_directed, 1)
    # a node that is no genome
    with pytest.raises(KeyError, match="extract_submatrix"):
        matrix_extend(whole.extract_submatrix(names[:10]), small_genomes[1:], _toy_directed, 1)
    with pytest.raises(ValueError):
        matrix_extend(whole, [], _toy_directed, 1)


def test_extend_keeps_a_similarity_matrix_a_similarity_matrix(small_genomes):
    sim = matrix_de_novo(small_genomes, _toy_directed, 1, as_distance=False)
    old = sim.extract_submatrix([g.name for g in small_genomes[3:17]])
    got = matrix_extend(old, small_genomes, _toy_directed, 1)
    assert not got.is_distance and set(np.diag(got.to_ndarray())) == {1.0}
    assert np.array_equal(got.to_ndarray(), sim.to_ndarray())


def test_launcher_is_refused_for_the_six_metrics(small_genomes, monkeypatch):
    """Under a launcher the rows fill is refused before any GPU call (the message says it is a one-GPU call)."""
    from phamclust_amd import cli
    monkeypatch.setenv("WORLD_SIZE", "2")
    old = matrix_de_novo(small_genomes[:5], _toy_directed, 1)
    with pytest.raises(RuntimeError, match="one-GPU call"):
        matrix_extend(old, small_genomes, cli.METRICS["jc"], 1)


def test_cli_extend_flag(tmp_path):
    import pathlib
    from phamclust_amd import cli
    f = tmp_path / "old_distance_matrix.tsv"
    assert cli.parse_args(["in.tsv", "out"]).extend is None and cli.DEFAULTS["extend"] is None
    assert cli.parse_args(["in.tsv", "out", "--extend", str(f)]).extend == pathlib.Path(f)
    assert cli.parse_args(["in.tsv", "out", "-x", str(f), "-m", "jc"]).extend == pathlib.Path(f)


def test_rows_fill_is_declared_and_bound(native_built):
    """Both exports are in the header, the library and the binding; the version says so."""
    import ctypes
    from phamclust_amd import hip
    assert {"pc_fill_rows", "pc_fill_rows_dev"} <= set(hip.EXPORTS)
    lib = hip.load()
    assert lib.pc_version() >= 155
    for twin in (hip.LIB_PATH, hip.LIB_PATH.replace("libphamclust_hip.so", "libphamclust_hip_hooks.so")):
        assert hasattr(ctypes.CDLL(twin), "pc_fill_rows") and hasattr(ctypes.CDLL(twin), "pc_fill_rows_dev")
    assert callable(hip.Context.fill_rows)
