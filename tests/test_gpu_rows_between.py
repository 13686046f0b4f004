"""The rows form of the between-groups fill (pc_fill_rows_between / Context.fill_rows_between / between_extend / --grow-table) on the GPU,
through real fills (run with ``-m gpu``).

Contract (a): seeded with the between-groups fill of the collection WITHOUT the query genomes, the call returns the between-groups fill
of the whole collection.  (b): without a seed and with every genome a query row it is that fill itself.  (c): without a seed it is the
table over exactly the pairs with a labelled query end and both ends labelled.  Every comparison is exact: ``np.array_equal`` on integer
arrays, byte equality on files."""

import re

import numpy as np
import pytest

from test_between_host import partitions
from test_gpu_between import golden_matrix, labels_of

pytestmark = pytest.mark.gpu

METRICS = ["jc", "peq"]
NAMES = ("sum", "count", "lo", "hi")
DTYPES = (np.int64, np.int64, np.int32, np.int32)
EMPTY_LO, EMPTY_HI = 2**31 - 1, -1
MILLION = 1000000
_SYNTH200 = []


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def genomes_of(name, small_genomes):
    """The fixture's genomes in fill order (synth200: the first 200 of synth(2000, 5000) by name, as conftest's synth200_packed packs them)."""
    if name == "small":
        return small_genomes
    if not _SYNTH200:
        from phamclust_amd.synth import synth_genomes
        _SYNTH200.append(sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:200])
    return _SYNTH200[0]


def row_sets(n):
    """One genome, genomes 0 and N - 1, a consecutive run of 5, every third genome."""
    return {"one": [n // 3], "ends": [0, n - 1], "run": list(range(n // 2, n // 2 + 5)), "third": list(range(1, n, 3))}


def same(got, want, label):
    for arr, ref, name, dtype in zip(got, want, NAMES, DTYPES):
        assert arr.dtype == dtype and arr.shape == np.asarray(ref).shape and np.array_equal(arr, ref), label + (name,)


def arrays_of(table):
    return (table.sum, table.cnt, table.lo, table.hi)


def query_end_table(matrix, label, rows, n_groups):
    """Plain numpy over the golden matrix: the table over the pairs {q, g} with q a query row, both labelled; a pair once."""
    micro = np.rint(matrix.to_ndarray() * 1.0e6).astype(np.int64)
    n = micro.shape[0]
    is_query = np.zeros(n, dtype=bool)
    is_query[list(rows)] = True
    total = np.zeros((n_groups, n_groups), dtype=np.int64)
    count = np.zeros((n_groups, n_groups), dtype=np.int64)
    lo = np.full((n_groups, n_groups), EMPTY_LO, dtype=np.int32)
    hi = np.full((n_groups, n_groups), EMPTY_HI, dtype=np.int32)
    for s in range(n):
        for t in range(s + 1, n):
            if (is_query[s] or is_query[t]) and label[s] >= 0 and label[t] >= 0:
                for a, b in {(label[s], label[t]), (label[t], label[s])}:
                    total[a, b] += micro[s, t]
                    count[a, b] += 1
                    lo[a, b] = min(lo[a, b], micro[s, t])
                    hi[a, b] = max(hi[a, b], micro[s, t])
    return total, count, lo, hi


def inverted(table):
    total, count, lo, hi = table
    full = count > 0
    return (count * MILLION - total, count, np.where(full, MILLION - hi.astype(np.int64), EMPTY_LO).astype(np.int32),
            np.where(full, MILLION - lo.astype(np.int64), EMPTY_HI).astype(np.int32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_a_seeded_call_is_the_whole_fill(ctx, small_genomes, name, metric):
    """Contract (a): fill_between over the old genomes alone as the seed; the grown table is fill_between over all genomes and
    GroupLinkage.from_dense of the golden matrix -- for four row sets, one slab and one row per slab, both directions."""
    from phamclust_amd.matrix import GroupLinkage
    from phamclust_amd.pack import pack_genomes
    genomes = genomes_of(name, small_genomes)
    matrix = golden_matrix(name, metric)
    names = matrix.nodes
    n = len(names)
    assert len(genomes) == n
    groups = partitions(matrix)["mod7" if name == "small" else "cc_mid"]
    label = labels_of(names, groups)
    g = len(groups)
    whole_packed = pack_genomes(genomes)
    dense = GroupLinkage.from_dense(matrix, groups)
    for tag, rows in row_sets(n).items():
        old = [k for k in range(n) if k not in set(rows)]
        ctx.upload(pack_genomes([genomes[k] for k in old]))
        seeds = {d: ctx.fill_between(metric, label[old], g, as_distance=d) for d in (True, False)}
        ctx.upload(whole_packed)
        for as_distance in (True, False):
            whole = ctx.fill_between(metric, label, g, as_distance=as_distance)
            same(whole, arrays_of(dense if as_distance else dense.inverted()), (name, metric, "the whole fill is the golden matrix's table"))
            for slab_bytes in (0, 8 * n * 1 + 7):
                *got, st = ctx.fill_rows_between(metric, label, rows, g, seed=seeds[as_distance], as_distance=as_distance, slab_bytes=slab_bytes,
                                                 want_stats=True)
                same(got, whole, (name, metric, tag, as_distance, slab_bytes))
                assert st["n_slabs"] == (len(rows) if slab_bytes else 1) and st["n_groups"] == g, (name, metric, tag, st["n_slabs"])
                assert st["ms_reduce"] > 0.0 and st["ms_finish"] > 0.0, (name, metric, tag)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_seedless_calls(ctx, small_packed, synth200_packed, name, metric):
    """Contracts (b) and (c): all rows without a seed is fill_between; a subset is the table over the pairs with a query end; with -1 on
    some queries and on one old genome it is that table over the labelled genomes -- stated by plain numpy over the golden matrix."""
    packed = small_packed if name == "small" else synth200_packed
    matrix = golden_matrix(name, metric)
    names = matrix.nodes
    n = len(names)
    ctx.upload(packed)
    groups = partitions(matrix)["mod7" if name == "small" else "blocks"]
    label = labels_of(names, groups)
    g = len(groups)
    for as_distance in (True, False):
        whole = ctx.fill_between(metric, label, g, as_distance=as_distance)
        for slab_bytes in (0, 8 * n * 9 + 7):
            same(ctx.fill_rows_between(metric, label, list(range(n)), g, as_distance=as_distance, slab_bytes=slab_bytes), whole,
                 (name, metric, "all rows", as_distance, slab_bytes))
    rows = sorted({0, 1, n // 2, n - 1} | set(range(3, n, 11)))
    loose = label.copy()
    loose[rows[1]] = loose[rows[-2]] = loose[2] = -1                         # two queries and genome 2, which is old, in no group
    assert 2 not in rows
    for tag, lab in (("labelled", label), ("unlabelled", loose)):
        want = query_end_table(matrix, lab, rows, g)
        assert want[1].sum() > 0 and (tag == "labelled" or want[1].sum() < query_end_table(matrix, label, rows, g)[1].sum())
        for as_distance in (True, False):
            for slab_bytes in (0, 8 * n):
                got = ctx.fill_rows_between(metric, lab, rows, g, as_distance=as_distance, slab_bytes=slab_bytes)
                same(got, want if as_distance else inverted(want), (name, metric, tag, as_distance, slab_bytes))


def test_seed_refusals_and_empty_cases(ctx, small_packed, small_genomes):
    """Each seed refusal once, naming the entry, and after each the context still fills correctly; pc_fill_between keeps refusing -1;
    n_rows == 0 returns the seed; N == 1 works."""
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    n = small_packed.n_genomes
    label = (np.arange(n, dtype=np.int32) * 5) % 3
    rows = [0, n // 2, n - 1]
    old = [k for k in range(n) if k not in rows]
    ctx.upload(pack_genomes([small_genomes[k] for k in old]))
    seed = ctx.fill_between("jc", label[old], 3)
    ctx.upload(small_packed)
    whole = ctx.fill_between("jc", label, 3)

    def broken(which, at, value):
        parts = [arr.copy() for arr in seed]
        for a, b in at:
            parts[which][a, b] = value(parts[which][a, b])
        return tuple(parts)

    both = lambda a, b: [(a, b), (b, a)]                                     # noqa: E731
    empty = tuple(np.full((3, 3), e, dtype=t) for e, t in zip((0, 0, EMPTY_LO, EMPTY_HI), DTYPES))
    refusals = [
        (broken(0, [(0, 1)], lambda v: v + 1), r"seed entry \[0\]\[1\].*is not symmetric"),
        (broken(1, both(0, 2), lambda v: v + 1), r"seed entry \[0\]\[2\] counts \d+ pairs, the partition has \d+ there"),
        (broken(1, [(1, 1)], lambda v: v - 1), r"seed entry \[1\]\[1\] counts"),
        (broken(2, both(1, 2), lambda v: seed[3][1, 2] + 1), r"seed entry \[1\]\[2\].*lo <= hi"),
        (broken(0, both(0, 0), lambda v: seed[1][0, 0] * (seed[3][0, 0] + 1)), r"seed entry \[0\]\[0\].*sum outside \[count lo, count hi\]"),
        (broken(0, both(2, 2), lambda v: -1), r"seed entry \[2\]\[2\].*sum outside"),
    ]
    for parts, text in refusals:
        with pytest.raises(hip.HipLibraryError, match=text):
            ctx.fill_rows_between("jc", label, rows, 3, seed=parts)
        same(ctx.fill_rows_between("jc", label, rows, 3, seed=seed), whole, ("after the refusal", text))
    # an empty entry with a non-zero sum: group 2 held by the queries alone
    only = np.where(np.isin(np.arange(n), rows), 2, np.arange(n) % 2).astype(np.int32)
    ctx.upload(pack_genomes([small_genomes[k] for k in old]))
    seed2 = ctx.fill_between("jc", only[old], 3)
    ctx.upload(small_packed)
    assert seed2[1][2].tolist() == [0, 0, 0]
    bad = [arr.copy() for arr in seed2]
    bad[0][0, 2] = bad[0][2, 0] = 5
    with pytest.raises(hip.HipLibraryError, match=r"seed entry \[0\]\[2\].*is neither empty .* nor full"):
        ctx.fill_rows_between("jc", only, rows, 3, seed=tuple(bad))
    same(ctx.fill_rows_between("jc", only, rows, 3, seed=seed2), ctx.fill_between("jc", only, 3), ("a group of queries alone",))
    # only three of the four seed pointers (below the binding, which insists on four)
    lib = ctx._lib
    import ctypes
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    cells = [i64p(), i64p(), i32p(), i32p()]
    nsl = ctypes.c_int32(9)
    prow = np.asarray(rows, dtype=np.int32)
    rc = lib.pc_fill_rows_between(ctx._h, hip.METRIC_IDS["jc"], 1, label.ctypes.data_as(i32p), 3, prow.ctypes.data_as(i32p), len(rows),
                                  seed[0].ctypes.data_as(i64p), seed[1].ctypes.data_as(i64p), seed[2].ctypes.data_as(i32p), None, 0,
                                  *(ctypes.byref(c) for c in cells), ctypes.byref(nsl), None)
    assert rc == -1 and b"3 of the four seed arrays" in lib.pc_last_error() and all(not c for c in cells) and nsl.value == 0
    same(ctx.fill_rows_between("jc", label, rows, 3, seed=seed), whole, ("after three seed pointers",))
    # the rows argument is refused before the seed; the whole form keeps refusing -1, the rows form admits it
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_rows_between: rows must be strictly ascending"):
        ctx.fill_rows_between("jc", label, [2, 1], 3, seed=refusals[0][0])
    unlabelled = label.copy()
    unlabelled[3] = -1
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_between: genome 3 has label -1"):
        ctx.fill_between("jc", unlabelled, 3)
    with pytest.raises(hip.HipLibraryError, match=r"pc_fill_rows_between: genome 3 has label -2"):
        ctx.fill_rows_between("jc", np.where(unlabelled < 0, -2, unlabelled), rows, 3)
    assert ctx.fill_rows_between("jc", unlabelled, [3], 3)[1].sum() == 0
    # no rows: the seed comes back (both directions), or an all-empty table
    *back, st = ctx.fill_rows_between("jc", label, [], 3, seed=whole, want_stats=True)
    same(back, whole, ("no rows: the seed",))
    assert st["n_slabs"] == 0
    sim = ctx.fill_between("jc", label, 3, as_distance=False)
    same(ctx.fill_rows_between("jc", label, [], 3, seed=sim, as_distance=False), sim, ("no rows: the similarity seed",))
    same(ctx.fill_rows_between("jc", label, [], 3), empty, ("no rows, no seed",))
    ctx.upload(pack_genomes(small_genomes[:1]))
    one = tuple(arr[:1, :1] for arr in empty)
    same(ctx.fill_rows_between("jc", np.zeros(1, dtype=np.int32), [0], 1), one, ("one genome",))
    same(ctx.fill_rows_between("jc", np.zeros(1, dtype=np.int32), [0], 1, seed=one), one, ("one genome, an empty seed",))
    with pytest.raises(hip.HipLibraryError, match=r"seed entry \[0\]\[0\]"):
        ctx.fill_rows_between("jc", np.zeros(1, dtype=np.int32), [], 1, seed=tuple(arr[:1, :1] for arr in whole))


def test_between_extend_equals_the_dense_route(small_genomes):
    """The route: the stored table of the old genomes grown by the new ones equals GroupLinkage.from_dense on the dense route's matrix;
    LAST_FILL is set; a stored table of another metric is refused by the verification, naming a group pair."""
    from phamclust_amd import matrix as pm
    from phamclust_amd import metrics
    func = {name: f for f, name in metrics.ACCELERATED.items()}
    names = [g.name for g in small_genomes]
    n = len(names)
    new = {2, 11, n - 1}
    old_genomes = [g for k, g in enumerate(small_genomes) if k not in new]
    old_names = [g.name for g in old_genomes]
    old_groups = [old_names[0::3], old_names[1::3], old_names[2::3]]
    grown = [old_groups[0] + [names[2]], old_groups[1], old_groups[2] + [names[11]], [names[n - 1]]]
    dense = pm.matrix_de_novo(small_genomes, func["jc"], 1)
    for as_distance in (True, False):
        stored = pm.between_de_novo(old_genomes, func["jc"], old_groups, as_distance=as_distance)
        for verify in (8, 0, 1):
            got = pm.between_extend(stored, small_genomes, func["jc"], grown, verify=verify)
            want = pm.GroupLinkage.from_dense(dense, [sorted(group, key=names.index) for group in grown])
            assert got == (want if as_distance else want.inverted()), (as_distance, verify)
            assert pm.LAST_FILL["metric"] == "jc" and pm.LAST_FILL["n_gpus"] == 1 and pm.LAST_FILL["rows"] == 3 and pm.LAST_FILL["n_slabs"] == 1
            assert pm.LAST_FILL["n_pairs"] < n * (n - 1) // 2
    other = pm.between_de_novo(old_genomes, func["gcs"], old_groups)
    with pytest.raises(ValueError, match=r"groups \d+ and \d+: the stored table holds \w+ \d+, the jc fill gives \d+: the file was not written with this metric"):
        pm.between_extend(other, small_genomes, func["jc"], grown)
    assert len(pm.between_extend(other, small_genomes, func["jc"], grown, verify=0)) == 4      # verify=0 skips the verification


def test_cli_grow_table_equals_the_dense_statement(small_genomes, tmp_path, monkeypatch):
    """--cluster-table --cluster-fit over the old genomes, then --place FIT --grow-table TABLE over all of them: cluster_table_jc.tsv
    is, byte for byte, the file of ``GroupLinkage.from_dense`` on the golden matrix over the grown groups; once more with --join-min
    high enough that a new genome becomes a singleton; a table of another metric exits 1 with the reason in the log and writes nothing."""
    from phamclust_amd import matrix as pm
    from phamclust_amd.scripts import phamclust as script
    from phamclust_amd.synth import write_tsv
    monkeypatch.setenv("PHAMCLUST_NO_HEATMAPS", "1")
    names = [g.name for g in small_genomes]
    new = [2, 11, len(names) - 1]
    all_tsv, old_tsv = tmp_path / "all.tsv", tmp_path / "old.tsv"
    write_tsv(small_genomes, all_tsv)
    write_tsv([g for k, g in enumerate(small_genomes) if k not in new], old_tsv)

    def run(name, tsv, *flags, metric="jc"):
        out = tmp_path / name
        script.main([str(tsv), str(out), "-m", metric, *flags])
        return out

    stored = run("old", old_tsv, "--cluster-table", "--cluster-fit")
    (fit,) = list(stored.rglob("cluster_fit_jc.tsv"))
    (table,) = list(stored.rglob("cluster_table_jc.tsv"))
    clusters, fit_groups, own = pm.stored_fit_from_file(fit)
    table_names, _ = pm.between_from_file(table, None, is_distance=False)
    assert sorted(table_names) == sorted(clusters)
    dense = golden_matrix("small", "jc")
    assert dense.nodes == names
    placement = pm.GroupPlacement.from_dense(dense, fit_groups, [names[k] for k in new])
    similarity = dict(zip(placement.queries, 1.0 - placement.nearest_value("mean")))
    assert not np.isnan(list(similarity.values())).any()
    cut = sorted(similarity.values())[1]                                     # the least similar new genome stays below it
    for tag, flags, join_min in (("grown", [], None), ("joined", ["--join-min", repr(float(cut))], float(cut))):
        out = run(tag, all_tsv, "--place", str(fit), "--grow-table", str(table), *flags)
        joined = placement.assigned("mean", min_similarity=join_min)
        groups = [list(fit_groups[clusters.index(name)]) for name in table_names]
        singles = []
        for k in new:
            if joined[names[k]] is None:
                singles.append(names[k])
            else:
                groups[table_names.index(clusters[joined[names[k]]])].append(names[k])
        assert len(singles) == (0 if join_min is None else 1), (tag, similarity, cut)
        want = pm.GroupLinkage.from_dense(dense, groups + [[x] for x in singles]).inverted()
        pm.between_to_file(want, table_names + singles, tmp_path / f"{tag}_want.tsv")
        assert (out / "cluster_table_jc.tsv").read_bytes() == (tmp_path / f"{tag}_want.tsv").read_bytes(), tag
        assert (out / "placement_jc.tsv").exists()
        log = (out / "phamclust.log").read_text()
        assert "grew the table of" in log and "wrote cluster_table_jc.tsv" in log
    # a table of another metric over the same clusters: the counts agree, the verification does not
    old_groups = [list(fit_groups[clusters.index(name)]) for name in table_names]
    pm.between_to_file(pm.GroupLinkage.from_dense(golden_matrix("small", "gcs"), old_groups).inverted(), table_names, tmp_path / "cluster_table_other.tsv")
    with pytest.raises(SystemExit) as exit_info:
        run("stale", all_tsv, "--place", str(fit), "--grow-table", str(tmp_path / "cluster_table_other.tsv"))
    assert exit_info.value.code == 1
    log = (tmp_path / "stale" / "phamclust.log").read_text()
    assert "--grow-table" in log and "the file was not written with this metric from these genomes" in log
    assert re.search(r"groups \d+ and \d+: the stored table holds \w+ \d+, the jc fill gives \d+", log)
    assert not (tmp_path / "stale" / "cluster_table_jc.tsv").exists()
    # a table with a group the fit file lacks
    text = (tmp_path / "cluster_table_other.tsv").read_text().replace(table_names[0] + "\t", "nobody\t")
    (tmp_path / "cluster_table_stranger.tsv").write_text(text)
    with pytest.raises(SystemExit):
        run("stranger", all_tsv, "--place", str(fit), "--grow-table", str(tmp_path / "cluster_table_stranger.tsv"))
    assert "--grow-table" in (tmp_path / "stranger" / "phamclust.log").read_text() and not (tmp_path / "stranger" / "cluster_table_jc.tsv").exists()
