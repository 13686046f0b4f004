"""The rows fill (pc_fill_rows / Context.fill_rows / matrix_extend / --extend) on the GPU (run with ``-m gpu``).

A rows fill must give, for every query row, exactly the cells the whole fill gives -- the pair in the whole fill's orientation
(aai is not symmetric), the diagonal as matrix_de_novo presets it -- on every row set, metric and direction, whatever the
chunking and the tie rule; its counters must cover each distinct pair once; and the container work above it (matrix_extend, the
CLI's --extend) must reproduce a straight run byte for byte and refuse a matrix that another metric filled."""


import numpy as np
import pytest
from scipy.spatial.distance import squareform

import planner_cases as pc
from conftest import ALL_METRICS, SET_METRICS, read_lower_triangle, synth200_file

pytestmark = pytest.mark.gpu
SEVEN = ALL_METRICS + ["aai_ppos"]


def row_sets(n):
    rng = np.random.default_rng(n)
    return {"first": [0], "last": [n - 1], "middle": [n // 2], "run": list(range(n // 3, n // 3 + 5)),
            "scattered": sorted(rng.choice(n, max(3, n // 6), replace=False).tolist()), "all": list(range(n))}


def square(condensed, n, as_distance):
    full = squareform(np.asarray(condensed), force="tomatrix", checks=False) if n > 1 else np.zeros((n, n))
    np.fill_diagonal(full, 1.0 - as_distance)                   # matrix.py:467-468
    return full


def distinct_pairs(rows, n):
    """(s, t), s < t, of the pairs {q, g}, q in rows, g != q, each once."""
    rows = set(rows)
    return sorted({(min(q, g), max(q, g)) for q in rows for g in range(n) if g != q})


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


_ORACLE = {}


def oracle_square(name, packed, metric, as_distance):
    """oracle.pairs over every pair of the collection, once per (collection, metric, direction)."""
    from oracle import oracle
    key = (name, metric, as_distance)
    if key not in _ORACLE:
        s, t = np.triu_indices(packed.n_genomes, k=1)
        _ORACLE[key] = square(oracle.pairs(packed, metric, s, t, as_distance), packed.n_genomes, as_distance)
    return _ORACLE[key]


@pytest.mark.parametrize("metric", SEVEN)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_rows_equal_the_whole_fill_and_the_oracle(ctx, small_packed, synth200_packed, name, metric):
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    for as_distance in (True, False):
        whole = square(ctx.fill(metric, as_distance), n, as_distance)
        want = oracle_square(name, packed, metric, as_distance)
        for label, rows in row_sets(n).items():
            got = ctx.fill_rows(metric, rows, as_distance)
            assert got.shape == (len(rows), n) and got.dtype == np.float64
            assert np.array_equal(got, whole[rows]), (name, metric, as_distance, label)
            assert np.array_equal(got, want[rows]), (name, metric, as_distance, label, "oracle")
        if name == "synth200" and metric in SET_METRICS and as_distance:          # the reference's own file
            _, condensed, _ = read_lower_triangle(synth200_file(metric))
            ref = square(condensed, n, True)
            for label, rows in row_sets(n).items():
                assert np.array_equal(ctx.fill_rows(metric, rows), ref[rows]), (metric, label, "reference file")


def test_a_middle_row_of_aai_runs_both_orientations(ctx, synth200_packed):
    """aai(s, t) != aai(t, s) for some pairs of the collection (the anchor rule, metrics.py:208-209), and a middle row is the
    target of the genomes before it and the source of those after it: both halves equal the whole fill."""
    from oracle import oracle
    n, q = synth200_packed.n_genomes, 100
    ctx.upload(synth200_packed)
    whole = square(ctx.fill("aai"), n, True)
    got = ctx.fill_rows("aai", [q])[0]
    assert np.array_equal(got[:q], whole[q, :q]) and np.array_equal(got[q + 1:], whole[q, q + 1:]) and got[q] == 0.0
    assert np.array_equal(np.delete(got, q), np.array([oracle.pair(synth200_packed, "aai", min(q, g), max(q, g)) for g in range(n) if g != q]))


def test_rows_fill_over_every_launch_class(ctx):
    """The designed collection of tests/planner_cases.py (every launch class a default process reaches, the strip-mined ones
    included): a rows fill over a scattered third of its genomes equals the whole fill's cells."""
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    C = hip.Context
    packed = pack_genomes(pc.build(pc.design(C)))
    n = packed.n_genomes
    rows = list(range(1, n, 3))
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    for metric, as_distance in (("aai", True), ("peq", True), ("peq", False), ("aai_ppos", True)):
        whole, st_whole = ctx.fill(metric, as_distance, want_stats=True)
        whole_tasks = ctx.last_plan_tasks()
        got, st = ctx.fill_rows(metric, rows, as_distance, want_stats=True)
        assert np.array_equal(got, square(whole, n, as_distance)[rows]), (metric, as_distance)
        tasks = ctx.last_plan_tasks()
        assert tasks.sum() == st["n_tasks"] > 0 and st["n_alignments"] < st_whole["n_alignments"]
        reached = [pc.class_name(C, int(k)) for k in np.flatnonzero(tasks)]
        print(f"{metric}: rows fill reaches {len(reached)} of the whole fill's {np.count_nonzero(whole_tasks)} launch classes")
        assert any("strip-mined" in x for x in reached) and any("one wave" in x for x in reached) and any("two waves" in x for x in reached)
        assert set(np.flatnonzero(tasks)) <= set(np.flatnonzero(whole_tasks))


def test_chunked_rows_fill_gives_the_same_values(ctx, synth200_packed):
    n = synth200_packed.n_genomes
    rows = sorted(set(row_sets(n)["scattered"]) | {0, n - 1})
    ctx.upload(synth200_packed)
    for metric in ("peq", "aai"):
        one, st1 = ctx.fill_rows(metric, rows, want_stats=True)
        assert st1["n_chunks"] == 1
        try:
            # a fifth of what the plan (56 bytes per alignment) and the slot arrays (8 bytes per slot) of the whole request take
            ctx.set_plan_budget((st1["n_alignments"] * 56 + len(rows) * n * 8) // 5)
            cut, st = ctx.fill_rows(metric, rows, want_stats=True)
            assert 5 <= st["n_chunks"] <= len(rows)
            ctx.set_plan_budget(56)                                    # one row per chunk
            single, st_single = ctx.fill_rows(metric, rows, want_stats=True)
            assert st_single["n_chunks"] == len(rows)
        finally:
            ctx.set_plan_budget(0)
        for other, st_other in ((cut, st), (single, st_single)):
            assert np.array_equal(other, one)
            for key in ("n_pairs", "n_alignments", "n_cells", "n_residue_bytes"):
                assert st_other[key] == st1[key], key
        assert np.array_equal(ctx.fill_rows(metric, rows), one)


def test_rows_fill_under_another_tie_rule(ctx, small_packed):
    from oracle import oracle
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    for rule in (0, 5):
        ctx.set_tie_rule(rule)
        whole = square(ctx.fill("aai"), n, True)
        for rows in row_sets(n).values():
            assert np.array_equal(ctx.fill_rows("aai", rows), whole[rows]), rule
        with oracle.tie_rule(rule):
            s, t = np.triu_indices(n, k=1)
            assert np.array_equal(whole, square(oracle.pairs(small_packed, "aai", s, t), n, True)), rule
    ctx.set_tie_rule(0)


@pytest.mark.parametrize("name", ["small", "synth200"])
def test_stats_cover_each_distinct_pair_once(ctx, small_packed, synth200_packed, name):
    from oracle import oracle
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    ctx.upload(packed)
    for label, rows in row_sets(n).items():
        m = len(rows)
        pairs = distinct_pairs(rows, n)
        assert len(pairs) == m * (n - 1) - m * (m - 1) // 2
        a_gene, b_gene, _ = oracle.enumerate_alignments(packed, [p[0] for p in pairs], [p[1] for p in pairs])
        lens = np.diff(packed.seq_off)
        for metric in ("peq", "jc"):
            _, st = ctx.fill_rows(metric, rows, want_stats=True)
            assert st["n_pairs"] == len(pairs), label
            assert st["n_chunks"] == 1 and st["ms_total"] > 0.0
            if metric == "peq":
                assert st["n_alignments"] == len(a_gene), label
                assert st["n_cells"] == int((lens[a_gene] * lens[b_gene]).sum()), label
                assert st["n_residue_bytes"] == int((lens[a_gene] + lens[b_gene]).sum()), label
                assert 0 < st["n_distinct_alignments"] <= st["n_alignments"]
            else:
                assert st["n_alignments"] == 0
    whole, st_whole = ctx.fill("peq", want_stats=True)
    _, st_all = ctx.fill_rows("peq", list(range(n)), want_stats=True)
    for key in ("n_pairs", "n_alignments", "n_cells", "n_residue_bytes", "n_distinct_alignments", "n_tasks"):
        assert st_all[key] == st_whole[key], key
    assert ctx.last_plan_tasks().sum() == st_all["n_tasks"]


def test_statuses(ctx, small_packed):
    import ctypes
    from phamclust_amd import hip
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    assert ctx.fill_rows("jc", []).shape == (0, n)                                  # n_rows == 0: PC_OK, nothing done
    for bad in ([5, 3], [3, 3], [0, n], [-1, 2], [n]):
        with pytest.raises(hip.HipLibraryError, match="status -1"):
            ctx.fill_rows("jc", bad)
    lib, h = ctx._lib, ctx._h
    rows = np.array([1, 2], dtype=np.int32)
    rows_p = rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    out = np.zeros((2, n))
    out_p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.pc_fill_rows(h, 1, 1, rows_p, 2, None, None) == -1                   # NULL out
    assert lib.pc_fill_rows(h, 7, 1, rows_p, 2, out_p, None) == -1                  # bad metric
    assert lib.pc_fill_rows(h, -1, 1, rows_p, 2, out_p, None) == -1
    assert lib.pc_fill_rows_dev(h, 1, 1, rows_p, 2, None, None, None) == -1
    assert lib.pc_fill_rows(h, 1, 1, rows_p, 2, out_p, None) == 0
    kernel_before = ctx.last_set_kernel()
    whole = square(ctx.fill("jc"), n, True)
    assert np.array_equal(out, whole[[1, 2]])
    assert ctx.last_set_kernel() is not None
    ctx.fill_rows("af", [0])                                                        # no selector: the last WHOLE fill stays on record
    assert ctx.last_set_launch()[0]["metric"] == "jc" and (kernel_before is None or ctx.last_set_kernel() is not None)
    # a sharded context
    try:
        ctx.set_shard(0, 2)
        with pytest.raises(hip.HipLibraryError, match="status -3"):
            ctx.fill_rows("jc", [0])
    finally:
        ctx.set_shard(0, 1)
    # aai before the residues are on the device
    ctx.upload(small_packed, residues=False)
    assert lib.pc_fill_rows(h, 4, 1, rows_p, 2, out_p, None) == -3
    assert lib.pc_fill_rows(h, 1, 1, rows_p, 2, out_p, None) == 0 and np.array_equal(out, whole[[1, 2]])
    assert np.array_equal(ctx.fill_rows("aai", [1, 2]), square(ctx.fill("aai"), n, True)[[1, 2]])      # the binding uploads them first
    # before any upload
    fresh = hip.Context(ctx.device_id)
    try:
        assert fresh._lib.pc_fill_rows(fresh._h, 1, 1, rows_p, 2, out_p, None) == -3
    finally:
        fresh.close()


# ---- matrix_extend and the CLI ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth300(native_built):
    from phamclust_amd.synth import synth_genomes
    genomes = sorted(synth_genomes(300, 1500, seed=77), key=lambda g: g.name)
    new = list(range(7, 300, 15))                                     # 20 new genomes, scattered in name order
    assert len(new) == 20
    return genomes, new


def test_matrix_extend_equals_de_novo(synth300):
    from phamclust_amd import cli, matrix as M
    genomes, new = synth300
    old_genomes = [g for k, g in enumerate(genomes) if k not in set(new)]
    wholes = {}
    for metric in ALL_METRICS:
        func = cli.METRICS[metric]
        whole = wholes[metric] = M.matrix_de_novo(genomes, func, 1)
        old = whole.extract_submatrix([g.name for g in old_genomes])
        got = M.matrix_extend(old, genomes, func, 1)
        assert got.nodes == whole.nodes and got.is_distance
        assert np.array_equal(got.to_ndarray(), whole.to_ndarray()), metric
        assert M.LAST_FILL["metric"] == metric and M.LAST_FILL["rows"] == 24 and M.LAST_FILL["n_genomes"] == 300
        assert M.LAST_FILL["genome_pairs"] == 24 * 299 - 24 * 23 // 2
        # the old matrix filled on its own, from the 280 genomes alone, is the same block: what a user really holds
        if metric in ("jc", "peq"):
            alone = M.matrix_de_novo(old_genomes, func, 1)
            assert np.array_equal(M.matrix_extend(alone, genomes, func, 1).to_ndarray(), whole.to_ndarray()), metric
    # similarities, and no guard
    sim = M.matrix_de_novo(genomes, cli.METRICS["af"], 1, as_distance=False)
    old = sim.extract_submatrix([g.name for g in old_genomes])
    got = M.matrix_extend(old, genomes, cli.METRICS["af"], 1, verify=0)
    assert not got.is_distance and np.array_equal(got.to_ndarray(), sim.to_ndarray()) and M.LAST_FILL["rows"] == 20
    # the guard: a matrix another metric filled
    old_jc = wholes["jc"].extract_submatrix([g.name for g in old_genomes])
    with pytest.raises(ValueError, match="not filled with this metric from these genomes in this order"):
        M.matrix_extend(old_jc, genomes, cli.METRICS["gcs"], 1)


def _tree(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file() and p.suffix != ".log"}


def test_cli_extend_reproduces_a_straight_run(synth300, tmp_path):
    from phamclust_amd.scripts.phamclust import main
    from phamclust_amd.synth import write_tsv
    genomes, new = synth300
    all_tsv, old_tsv = tmp_path / "all.tsv", tmp_path / "old.tsv"
    write_tsv(genomes, all_tsv)
    write_tsv([g for k, g in enumerate(genomes) if k not in set(new)], old_tsv)

    def run(name, tsv, metric, *extra):
        out = tmp_path / name
        main([str(tsv), str(out), "-m", metric, "-t", "1", *extra])
        (cache,) = list(out.glob(f"*.tmp/02_distmats/{metric}_distance_matrix.tsv"))
        return out, cache

    _, old_cache = run("old", old_tsv, "jc")
    straight, straight_cache = run("straight", all_tsv, "jc")
    extended, extended_cache = run("extended", all_tsv, "jc", "--extend", str(old_cache))
    assert extended_cache.read_bytes() == straight_cache.read_bytes()
    a, b = _tree(extended), _tree(straight)
    assert sorted(a) == sorted(b)
    # byte for byte, but for the heatmap renderings: plotly writes random element ids into every .svg / .html, so two straight
    # runs differ there too (tests/test_pipeline.py leaves them out for the same reason); their presence is held above
    assert [rel for rel in a if a[rel] != b[rel] and not rel.endswith((".svg", ".html"))] == []
    assert sum(rel.endswith(".tsv") for rel in a) > 10 and sum(rel.endswith(".faa") for rel in a) == 300
    log = (extended / "phamclust.log").read_text()
    assert "extended 280 -> 300 genomes: 24 rows, " in log and "pairs filled instead of 44,850" in log
    # --gpus N with --extend: the matrix stage stays on one GPU and the log says why
    multi, multi_cache = run("multi", all_tsv, "jc", "--extend", str(old_cache), "--gpus", "2")
    assert multi_cache.read_bytes() == straight_cache.read_bytes()
    assert "one-GPU call" in (multi / "phamclust.log").read_text()
    # a matrix another metric filled: exit status 1, and the message
    _, gcs_cache = run("old_gcs", old_tsv, "gcs")
    with pytest.raises(SystemExit) as exit_info:
        run("wrong", all_tsv, "jc", "--extend", str(gcs_cache))
    assert exit_info.value.code == 1
    assert "not filled with this metric" in (tmp_path / "wrong" / "phamclust.log").read_text()
