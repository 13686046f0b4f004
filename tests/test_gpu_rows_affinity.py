"""The rows form of the affinity fill (pc_fill_rows_affinity / Context.fill_rows_affinity / placement_de_novo) on the GPU, through real
fills (run with ``-m gpu``).

With every genome labelled a query's entries are entry rows[k] of the whole affinity fill's, integer for integer, for any subset of rows
and any slab cut; with unlabelled queries the expected result comes from the golden dense matrix through ``GroupPlacement.from_dense``,
which tests/test_placement_host.py holds to plain loops; the gain is held to its identity -- the own entries of an affinity fill of the
collection WITHOUT the queries, grown by it, are the own entries of the affinity fill of the whole collection.  Every comparison is
exact: ``np.array_equal`` on integer arrays."""

import numpy as np
import pytest

from test_between_host import partitions
from test_gpu_between import golden_matrix, labels_of

pytestmark = pytest.mark.gpu

ARRAYS = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")
DTYPES = dict(own_sum=np.int64, own_lo=np.int32, own_hi=np.int32, near_group=np.int32, near_sum=np.int64, near_lo=np.int32, near_hi=np.int32)
TRIPLE = (np.int64, np.int32, np.int32)
METRICS = ["jc", "peq"]


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def row_sets(n):
    """One genome, genomes 0 and N - 1, a consecutive run, all N."""
    return {"one": [n // 3], "ends": [0, n - 1], "run": list(range(n // 2, min(n // 2 + 5, n))), "all": list(range(n))}


def check_rows_of_whole(got, whole, rows, label):
    """``got`` (a rows form's dict) against rows ``rows`` of a whole affinity fill's dict."""
    rows = np.asarray(rows, dtype=np.int64)
    for name in ARRAYS:
        ref = whole[name][:, rows] if name == "near_group" else whole[name][rows]
        assert got[name].dtype == DTYPES[name] and got[name].shape == ref.shape and np.array_equal(got[name], ref), (label, name)
    for arr, ref, dtype in zip(got["table"], whole["table"], TRIPLE):
        assert arr.dtype == dtype and arr.shape == ref[rows].shape and np.array_equal(arr, ref[rows]), (label, "table")


def check_placement(got, want, label):
    """``got`` (a rows form's dict) against a GroupPlacement."""
    for name in ARRAYS:
        ref = getattr(want, name)
        assert got[name].dtype == ref.dtype and got[name].shape == ref.shape and np.array_equal(got[name], ref), (label, name)
    for part in ("table", "gain"):
        for arr, ref in zip(got[part], getattr(want, part)):
            assert arr.dtype == ref.dtype and arr.shape == ref.shape and np.array_equal(arr, ref), (label, part)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_labelled_queries_are_the_whole_fills_rows(ctx, small_packed, synth200_packed, name, metric):
    """Every genome labelled: any subset of rows, in one slab and one row per slab, both directions, equals the whole fill row for row;
    the gain of an old genome is the part of its own entry that lies with the queries (checked against the dense matrix)."""
    from phamclust_amd.matrix import GroupPlacement
    packed = small_packed if name == "small" else synth200_packed
    matrix = golden_matrix(name, metric)
    names = matrix.nodes
    n = len(names)
    ctx.upload(packed)
    groups = partitions(matrix)["mod7" if name == "small" else "cc_mid"]
    label = labels_of(names, groups)
    for as_distance in (True, False):
        whole = ctx.fill_affinity(metric, label, len(groups), as_distance=as_distance, want_table=True)
        for tag, rows in row_sets(n).items():
            per = 1 if len(rows) <= 64 else 9                               # one row per slab; of many rows, nine (and 7 bytes that buy no row)
            for slab_bytes in (0, 8 * n * per + 7):
                got = ctx.fill_rows_affinity(metric, label, rows, len(groups), as_distance=as_distance, slab_bytes=slab_bytes, want_table=True, want_gain=True,
                                             want_stats=True)
                st = got.pop("stats")
                check_rows_of_whole(got, whole, rows, (name, metric, tag, as_distance, slab_bytes))
                assert st["n_slabs"] == ((len(rows) + per - 1) // per if slab_bytes else 1) and st["n_groups"] == len(groups), (name, metric, tag, st["n_slabs"])
                assert st["ms_rows"] > 0.0 and st["ms_cols"] > 0.0 and st["ms_finish"] > 0.0, (name, metric, tag)
                want = GroupPlacement.from_dense(matrix, groups, [names[r] for r in rows])
                check_placement(got, want if as_distance else want.inverted(), (name, metric, tag, as_distance, slab_bytes, "from_dense"))
        plain = ctx.fill_rows_affinity(metric, label, [0, n - 1], len(groups), as_distance=as_distance)
        assert plain["table"] is None and plain["gain"] is None
        for key in ARRAYS:
            ref = whole[key][:, [0, n - 1]] if key == "near_group" else whole[key][[0, n - 1]]
            assert np.array_equal(plain[key], ref), (name, metric, as_distance, key, "no table, no gain")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_unlabelled_queries_equal_the_dense_statement(ctx, small_packed, synth200_packed, name, metric):
    """Query labels -1 (and one old genome in no group): the statement of the oracle's matrix, under both slab cuts and directions."""
    from phamclust_amd.matrix import GroupPlacement
    packed = small_packed if name == "small" else synth200_packed
    matrix = golden_matrix(name, metric)
    names = matrix.nodes
    n = len(names)
    ctx.upload(packed)
    for tag, groups in partitions(matrix).items():
        if tag == "singletons" and n > 64:
            continue
        rows = sorted({0, 1, n // 2, n - 1} | set(range(3, n, 11)))
        loose = set(rows[:-1]) | {2}                                        # the last query keeps its label; genome 2 is old and in no group
        kept = [[x for x in group if names.index(x) not in loose] for group in groups]
        label = np.full(n, -1, dtype=np.int32)
        for b, group in enumerate(kept):
            label[[names.index(x) for x in group]] = b
        want = GroupPlacement.from_dense(matrix, kept, [names[r] for r in rows])
        assert (want.own_lo[:-1] == 2**31 - 1).all() and (want.near_group[0] >= 0).any()
        for as_distance in (True, False):
            for slab_bytes in (0, 8 * n):
                got = ctx.fill_rows_affinity(metric, label, rows, len(kept), as_distance=as_distance, slab_bytes=slab_bytes, want_table=True, want_gain=True)
                check_placement(got, want if as_distance else want.inverted(), (name, metric, tag, as_distance, slab_bytes))


@pytest.mark.parametrize("metric", METRICS)
def test_the_gain_grows_a_stored_affinity(ctx, small_genomes, metric):
    """own of an affinity fill of the uploaded sub-collection (+) gain == own of the affinity fill of the whole collection; the queries'
    own entries come from the rows form itself."""
    from phamclust_amd.pack import pack_genomes
    n = len(small_genomes)
    label = (np.arange(n, dtype=np.int32) * 5) % 3
    rows = sorted({0, n // 2, n // 2 + 1, n - 1})
    old = [g for g in range(n) if g not in rows]
    for as_distance in (True, False):
        ctx.upload(pack_genomes([small_genomes[g] for g in old]))
        stored = ctx.fill_affinity(metric, label[old], 3, as_distance=as_distance)
        ctx.upload(pack_genomes(small_genomes))
        whole = ctx.fill_affinity(metric, label, 3, as_distance=as_distance)
        for slab_bytes in (0, 8 * n):
            got = ctx.fill_rows_affinity(metric, label, rows, 3, as_distance=as_distance, slab_bytes=slab_bytes, want_gain=True)
            g_sum, g_lo, g_hi = got["gain"]
            assert np.array_equal(stored["own_sum"] + g_sum[old], whole["own_sum"][old]), (metric, as_distance, slab_bytes)
            assert np.array_equal(np.minimum(stored["own_lo"], g_lo[old]), whole["own_lo"][old]), (metric, as_distance, slab_bytes)
            assert np.array_equal(np.maximum(stored["own_hi"], g_hi[old]), whole["own_hi"][old]), (metric, as_distance, slab_bytes)
            assert (g_sum[rows] == 0).all() and (g_lo[rows] == 2**31 - 1).all() and (g_hi[rows] == -1).all()
            assert np.array_equal(got["own_sum"], whole["own_sum"][rows]) and g_sum[old].any()


def test_no_rows_one_genome_and_refusals(ctx, small_packed, small_genomes):
    """n_rows == 0 and N == 1: PC_OK with every entry empty.  The refusals come in the whole fill's order, then rows, leave the outputs
    alone and the context usable; pc_fill_affinity keeps refusing -1."""
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    label = np.arange(n, dtype=np.int32) % 4
    got = ctx.fill_rows_affinity("jc", label, [], 4, want_table=True, want_gain=True, want_stats=True)
    assert got["own_sum"].shape == (0,) and got["near_group"].shape == (3, 0) and got["table"][0].shape == (0, 4) and got["stats"]["n_slabs"] == 0
    assert (got["gain"][0] == 0).all() and (got["gain"][1] == 2**31 - 1).all() and (got["gain"][2] == -1).all() and got["gain"][0].shape == (n,)
    unlabelled = label.copy()
    unlabelled[3] = -1
    with pytest.raises(hip.HipLibraryError, match=r"genome 3 has label -1"):
        ctx.fill_affinity("jc", unlabelled, 4)
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_rows_affinity: genome 3 has label -2"):
        ctx.fill_rows_affinity("jc", np.where(unlabelled < 0, -2, unlabelled), [1], 4)
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_rows_affinity: n_groups 0"):
        ctx.fill_rows_affinity("jc", label, [1], 0)
    with pytest.raises(hip.HipLibraryError, match=r"n_groups 2049 is above"):
        ctx.fill_rows_affinity("jc", label, [1], 2049)
    for rows in ([1, 1], [2, 1], [n], [-1]):
        with pytest.raises(hip.HipLibraryError, match=r"pc_fill_rows_affinity: rows must be strictly ascending"):
            ctx.fill_rows_affinity("jc", label, rows, 4)
    with pytest.raises(hip.HipLibraryError, match=r"slab_bytes -1"):
        ctx.fill_rows_affinity("jc", label, [1], 4, slab_bytes=-1)
    ok = ctx.fill_rows_affinity("jc", unlabelled, [3], 4)
    assert ok["own_lo"][0] == 2**31 - 1 and ok["near_group"][0, 0] >= 0
    ctx.upload(pack_genomes(small_genomes[:1]))
    one = ctx.fill_rows_affinity("jc", np.zeros(1, dtype=np.int32), [0], 1, want_table=True, want_gain=True)
    assert one["own_sum"].tolist() == [0] and one["own_lo"].tolist() == [2**31 - 1] and one["near_group"].tolist() == [[-1]] * 3
    assert [arr.tolist() for arr in one["table"]] == [[[0]], [[2**31 - 1]], [[-1]]] and [arr.tolist() for arr in one["gain"]] == [[0], [2**31 - 1], [-1]]


def test_placement_de_novo_equals_the_dense_route(small_genomes):
    """The route: default queries (the genomes in no group), LAST_FILL, and the dense route's statement."""
    from phamclust_amd import matrix as pm
    from phamclust_amd import metrics
    func = next(f for f, name in metrics.ACCELERATED.items() if name == "jc")
    names = [g.name for g in small_genomes]
    groups = [names[0:5], names[5:9], [], names[9:-3]]
    dense = pm.matrix_de_novo(small_genomes, func, 1)
    for as_distance in (True, False):
        got = pm.placement_de_novo(small_genomes, func, groups, as_distance=as_distance, want_table=True, want_gain=True)
        want = pm.GroupPlacement.from_dense(dense, groups, names[-3:])
        assert got == (want if as_distance else want.inverted())
        assert pm.LAST_FILL["metric"] == "jc" and pm.LAST_FILL["n_gpus"] == 1 and pm.LAST_FILL["n_slabs"] == 1
    some = pm.placement_de_novo(small_genomes, func, groups, queries=[names[2], 7])
    assert some.queries == [names[2], names[7]] and some.table is None and some.gain is None
    assert some == pm.GroupPlacement.from_dense(dense, groups, [names[2], names[7]], want_table=False, want_gain=False)


def test_cli_place_equals_the_dense_statement(small_genomes, tmp_path, monkeypatch):
    """--cluster-fit over the old genomes, then --place over all of them: placement_jc.tsv is, byte for byte, the report of
    ``GroupPlacement.from_dense`` on the golden dense matrix; a file of another metric and a file whose genome is missing are refused,
    naming the genome."""
    from phamclust_amd import matrix as pm
    from phamclust_amd.scripts import phamclust as script
    from phamclust_amd.synth import write_tsv
    monkeypatch.setenv("PHAMCLUST_NO_HEATMAPS", "1")
    names = [g.name for g in small_genomes]
    new = {2, 11, len(names) - 1}
    all_tsv, old_tsv, fewer_tsv = tmp_path / "all.tsv", tmp_path / "old.tsv", tmp_path / "fewer.tsv"
    write_tsv(small_genomes, all_tsv)
    write_tsv([g for k, g in enumerate(small_genomes) if k not in new], old_tsv)
    write_tsv([g for k, g in enumerate(small_genomes) if k != 5], fewer_tsv)

    def run(name, tsv, *flags, metric="jc"):
        out = tmp_path / name
        script.main([str(tsv), str(out), "-m", metric, *flags])
        return out

    stored = run("old", old_tsv, "--cluster-fit")
    (fit,) = list(stored.rglob("cluster_fit_jc.tsv"))
    placed = run("placed", all_tsv, "--place", str(fit))
    clusters, groups, own = pm.stored_fit_from_file(fit)
    dense = golden_matrix("small", "jc")
    assert dense.nodes == names and sorted(own) == sorted(names[k] for k in range(len(names)) if k not in new)
    want = pm.GroupPlacement.from_dense(dense, groups, [names[k] for k in sorted(new)])
    assert (placed / "placement_jc.tsv").read_text() == "\n".join(pm.placement_report(want, clusters)) + "\n"
    assert not list(placed.rglob("cluster_fit_*")) and not list(placed.rglob("*similarities*"))
    log = (placed / "phamclust.log").read_text()
    assert f"placed 3 new genomes against {len(groups)} clusters of {len(names) - 3} genomes (" in log and "0 of them verified" not in log
    for name, tsv, metric, text in (("stale", all_tsv, "gcs", "the file was not written with this metric from these genomes"),
                                    ("missing", fewer_tsv, "jc", f"genome '{names[5]}' of the file is not among the genomes of the input")):
        with pytest.raises(SystemExit):
            run(name, tsv, "--place", str(fit), metric=metric)
        log = (tmp_path / name / "phamclust.log").read_text()
        assert text in log and "--place" in log and not (tmp_path / name / f"placement_{metric}.tsv").exists(), name
