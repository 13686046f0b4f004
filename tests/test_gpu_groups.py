"""The groups fill (pc_fill_groups / Context.fill_groups / submatrices_de_novo / --no-matrix) on the GPU (run with ``-m gpu``).

A groups fill must give, for every group, exactly the cells the whole fill gives for the group's genomes -- each pair in the whole
fill's orientation (aai is not symmetric) -- on every family of groups, metric and direction, whatever the chunking; its counters
are summed over the slots while its plan merges duplicate sequence pairs across groups; and the work above it (submatrices_de_novo,
hierarchical_clustering_de_novo, the CLI's --no-matrix) must reproduce the dense route."""

import json
import os

import numpy as np
import pytest
from scipy.spatial.distance import squareform

import planner_cases as pc
from conftest import ALL_METRICS, REPO, SET_METRICS, read_lower_triangle, synth200_file
from test_gpu_rows import oracle_square              # the oracle's squares, computed once per session for both modules

pytestmark = pytest.mark.gpu
SEVEN = ALL_METRICS + ["aai_ppos"]


def square(condensed, n, as_distance):
    full = squareform(np.asarray(condensed), force="tomatrix", checks=False) if n > 1 else np.zeros((n, n))
    np.fill_diagonal(full, 1.0 - as_distance)                   # matrix.py:467-468
    return full


def condensed_of(full, group):
    """The condensed vector (scipy order) of the block of ``full`` over ``group``."""
    group = np.asarray(group, dtype=np.int64)
    i, j = np.triu_indices(len(group), k=1)
    return full[group[i], group[j]]


def scattered(rng, n, size):
    return sorted(rng.choice(n, size, replace=False).tolist())


def families(n):
    """Families of groups over n genomes (23 or 200): every tiling case of the issue that fits."""
    rng = np.random.default_rng(n)
    out = {"everything": [list(range(n))], "singletons": [[g] for g in range(n)], "ends": [[0, n - 1]],
           "forty pairs": [sorted(rng.choice(n, 2, replace=False).tolist()) for _ in range(40)],
           "empty between": [scattered(rng, n, 3), [], scattered(rng, n, 4)],
           "overlapping": [list(range(2, min(n, 20))), list(range(10, min(n, 23), 2)) + ([n - 1] if n > 23 else [])]}
    if n >= 65:
        for size in (31, 32, 33, 65):
            out[f"scattered {size}"] = [scattered(rng, n, size)]
        out["30 + 5 straddling"] = [scattered(rng, n, 30), scattered(rng, n, 5)]
    else:
        out["20 + 15 straddling"] = [scattered(rng, n, 20), scattered(rng, n, 15)]         # the second group straddles position 32
    return out


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


@pytest.mark.parametrize("metric", SEVEN)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_groups_equal_the_whole_fill_and_the_oracle(ctx, small_packed, synth200_packed, name, metric):
    from phamclust_amd.matrix import Components
    packed = small_packed if name == "small" else synth200_packed
    n = packed.n_genomes
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    for as_distance in (True, False):
        flat = np.array(ctx.fill(metric, as_distance))
        whole = square(flat, n, as_distance)
        want = oracle_square(name, packed, metric, as_distance)
        cases = families(n)
        if as_distance:                                          # the components of a real threshold
            labels = ctx.fill_components(metric, 0.75 if name == "small" else float(np.quantile(flat, 0.02)))
            cases["components"] = [g.tolist() for g in Components([str(k) for k in range(n)], labels).group_indices()]
            assert 1 < len(cases["components"]) < n, "the threshold must give a real partition"
        for label, groups in cases.items():
            got = ctx.fill_groups(metric, groups, as_distance)
            assert len(got) == len(groups)
            for group, values in zip(groups, got):
                assert values.dtype == np.float64 and values.shape == (len(group) * (len(group) - 1) // 2,)
                assert np.array_equal(values, condensed_of(whole, group)), (name, metric, as_distance, label)
                assert np.array_equal(values, condensed_of(want, group)), (name, metric, as_distance, label, "oracle")
        assert np.array_equal(ctx.fill_groups(metric, [list(range(n))], as_distance)[0], flat)      # one group of everything: the whole vector
        assert sum(v.size for v in ctx.fill_groups(metric, cases["singletons"], as_distance)) == 0
        if name == "synth200" and metric in SET_METRICS and as_distance:          # the reference's own file
            _, condensed, _ = read_lower_triangle(synth200_file(metric))
            ref = square(condensed, n, True)
            for label, groups in cases.items():
                for group, values in zip(groups, ctx.fill_groups(metric, groups)):
                    assert np.array_equal(values, condensed_of(ref, group)), (metric, label, "reference file")


def test_aai_keeps_the_whole_fills_orientation(ctx, synth200_packed):
    """aai(s, t) != aai(t, s) for some pairs of the collection (the anchor rule, metrics.py:208-209).  A group whose members
    interleave with non-members must give such pairs the value of (smaller index, larger index), not the other one.  The other
    orientation comes from the oracle over the same genomes packed in reverse order: there the pair's roles are swapped."""
    from oracle import oracle
    from phamclust_amd.pack import pack_genomes
    from phamclust_amd.synth import synth_genomes
    n = synth200_packed.n_genomes
    reverse_packed = pack_genomes(sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:n][::-1])
    assert reverse_packed.names == synth200_packed.names[::-1]
    ctx.upload(synth200_packed)
    whole = square(ctx.fill("aai"), n, True)
    group = list(range(1, n, 3))
    i, j = np.triu_indices(len(group), k=1)
    s, t = np.asarray(group)[i], np.asarray(group)[j]
    forward = np.asarray(oracle.pairs(synth200_packed, "aai", s, t, True))
    backward = np.asarray(oracle.pairs(reverse_packed, "aai", n - 1 - t, n - 1 - s, True))
    asymmetric = np.flatnonzero(forward != backward)
    assert asymmetric.size > 0, "the collection must hold pairs on which the orientation shows"
    (got,) = ctx.fill_groups("aai", [group])
    assert np.array_equal(got[asymmetric], whole[s, t][asymmetric]) and np.array_equal(got[asymmetric], forward[asymmetric])
    assert (got[asymmetric] != backward[asymmetric]).all()
    assert np.array_equal(got, forward)


def test_groups_fill_over_every_launch_class(ctx):
    """The designed collection of tests/planner_cases.py (every launch class a default process reaches, the strip-mined ones
    included): the three groups i mod 3 equal the whole fill's cells."""
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    C = hip.Context
    packed = pack_genomes(pc.build(pc.design(C)))
    n = packed.n_genomes
    groups = [list(range(r, n, 3)) for r in range(3)]
    ctx.upload(packed)
    ctx.set_shard(0, 1)
    for metric, as_distance in (("aai", True), ("peq", True), ("peq", False), ("aai_ppos", True)):
        whole = square(ctx.fill(metric, as_distance), n, as_distance)
        got, st = ctx.fill_groups(metric, groups, as_distance, want_stats=True)
        for group, values in zip(groups, got):
            assert np.array_equal(values, condensed_of(whole, group)), (metric, as_distance)
        tasks = ctx.last_plan_tasks()
        assert tasks.sum() == st["n_tasks"] > 0
        reached = [pc.class_name(C, int(k)) for k in np.flatnonzero(tasks)]
        assert any("strip-mined" in x for x in reached) and any("one wave" in x for x in reached) and any("two waves" in x for x in reached)


def test_chunked_groups_fill_gives_the_same_values(ctx, synth200_packed):
    n = synth200_packed.n_genomes
    rng = np.random.default_rng(3)
    groups = [scattered(rng, n, 70), scattered(rng, n, 33), [5], scattered(rng, n, 40), [0, n - 1]]
    n_slots = sum(len(g) * (len(g) - 1) // 2 for g in groups)
    n_blocks = -(-sum(len(g) for g in groups) // 32)
    ctx.upload(synth200_packed)
    for metric in ("peq", "aai"):
        one, st1 = ctx.fill_groups(metric, groups, want_stats=True)
        assert st1["n_chunks"] == 1 and st1["n_pairs"] == n_slots
        try:
            # a fifth of what the plan (56 bytes per alignment) and the slot arrays (8 bytes per slot) of the whole request take
            ctx.set_plan_budget((st1["n_alignments"] * 56 + n_slots * 8) // 5)
            cut, st = ctx.fill_groups(metric, groups, want_stats=True)
            assert 1 < st["n_chunks"] <= n_blocks
            ctx.set_plan_budget(56)                                    # one row block per chunk
            single, st_single = ctx.fill_groups(metric, groups, want_stats=True)
            assert st["n_chunks"] <= st_single["n_chunks"] <= n_blocks and st_single["n_chunks"] > 1
        finally:
            ctx.set_plan_budget(0)
        for other, st_other in ((cut, st), (single, st_single)):
            for a, b in zip(other, one):
                assert np.array_equal(a, b)
            for key in ("n_pairs", "n_alignments", "n_cells", "n_residue_bytes"):
                assert st_other[key] == st1[key], key
        for a, b in zip(ctx.fill_groups(metric, groups), one):
            assert np.array_equal(a, b)


def test_duplicate_alignments_merge_across_groups(ctx, synth200_packed):
    """Counters are summed over the slots -- a pair in two groups counts twice -- while ONE plan serves all groups: the same
    sequence pairs, aligned once."""
    from oracle import oracle
    n = synth200_packed.n_genomes
    group = scattered(np.random.default_rng(9), n, 25)
    ctx.upload(synth200_packed)
    (a,), st1 = ctx.fill_groups("peq", [group], want_stats=True)
    (b, c), st2 = ctx.fill_groups("peq", [group, group], want_stats=True)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for key in ("n_pairs", "n_alignments", "n_cells", "n_residue_bytes"):
        assert st2[key] == 2 * st1[key] > 0, key
    assert st2["n_distinct_alignments"] == st1["n_distinct_alignments"] > 0
    assert st2["n_distinct_cells"] == st1["n_distinct_cells"] and st2["n_tasks"] == st1["n_tasks"]
    i, j = np.triu_indices(len(group), k=1)
    a_gene, b_gene, _ = oracle.enumerate_alignments(synth200_packed, np.asarray(group)[i], np.asarray(group)[j])
    lens = np.diff(synth200_packed.seq_off)
    assert st1["n_alignments"] == len(a_gene) and st1["n_cells"] == int((lens[a_gene] * lens[b_gene]).sum())
    assert st1["n_residue_bytes"] == int((lens[a_gene] + lens[b_gene]).sum())
    _, st_jc = ctx.fill_groups("jc", [group, group], want_stats=True)
    assert st_jc["n_pairs"] == st2["n_pairs"] and st_jc["n_alignments"] == 0 and st_jc["n_chunks"] == 1 and st_jc["ms_total"] > 0.0


def test_statuses(ctx, small_packed):
    import ctypes
    from phamclust_amd import hip
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    ctx.set_tie_rule(5)
    whole_jc = square(ctx.fill("jc"), n, True)
    whole_aai = square(ctx.fill("aai"), n, True)
    assert ctx.fill_groups("jc", []) == [] and [v.size for v in ctx.fill_groups("jc", [[], [3], []])] == [0, 0, 0]
    for bad in ([[5, 3]], [[3, 3]], [[0, n]], [[-1, 2]], [[1, 2], [n]]):                  # not ascending; twice; out of range (also in a group of one)
        with pytest.raises(hip.HipLibraryError, match="status -1"):
            ctx.fill_groups("jc", bad)
    lib, h = ctx._lib, ctx._h
    i32p, i64p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    members = np.array([1, 2, 7], dtype=np.int32)
    off = np.array([0, 3], dtype=np.int64)
    out = np.full(3, -1.0)
    m_p, o_p, out_p = members.ctypes.data_as(i32p), off.ctypes.data_as(i64p), out.ctypes.data_as(f64p)

    def offsets(*values):
        arr = np.array(values, dtype=np.int64)
        return arr, arr.ctypes.data_as(i64p)
    assert lib.pc_fill_groups(h, 1, 1, m_p, o_p, 1, None, None) == -1                     # NULL out, members, group_off with L > 0
    assert lib.pc_fill_groups(h, 1, 1, None, o_p, 1, out_p, None) == -1
    assert lib.pc_fill_groups(h, 1, 1, m_p, None, 1, out_p, None) == -1
    assert lib.pc_fill_groups_dev(h, 1, 1, m_p, o_p, 1, None, None, None) == -1
    assert lib.pc_fill_groups(h, 7, 1, m_p, o_p, 1, out_p, None) == -1                    # bad metric
    assert lib.pc_fill_groups(h, -1, 1, m_p, o_p, 1, out_p, None) == -1
    assert lib.pc_fill_groups(h, 1, 1, m_p, o_p, -1, out_p, None) == -1
    assert lib.pc_fill_groups(h, 1, 1, m_p, offsets(1, 3)[1], 1, out_p, None) == -1       # group_off[0] != 0
    assert lib.pc_fill_groups(h, 1, 1, m_p, offsets(0, 3, 2)[1], 2, out_p, None) == -1    # group_off decreasing
    assert lib.pc_fill_groups(h, 1, 1, m_p, offsets(0, 2 ** 31)[1], 1, out_p, None) == -1     # M > 2^31-1 (refused before a member is read)
    assert (out == -1.0).all()
    assert lib.pc_fill_groups(h, 1, 1, None, None, 0, None, None) == 0                    # n_groups == 0 and L == 0: PC_OK, nothing written
    assert lib.pc_fill_groups(h, 1, 1, m_p, offsets(0, 1, 2, 3)[1], 3, None, None) == 0
    assert lib.pc_fill_groups(h, 1, 1, m_p, o_p, 1, out_p, None) == 0
    assert np.array_equal(out, condensed_of(whole_jc, [1, 2, 7]))
    ctx.fill("jc")
    ctx.fill_groups("af", [[0, 1]])                                                       # no selector: the last WHOLE fill stays on record
    assert ctx.last_set_launch()[0]["metric"] == "jc"
    # a sharded context: refused, and the shard state stays
    try:
        ctx.set_shard(1, 2)
        pairs = ctx.shard_pairs()
        with pytest.raises(hip.HipLibraryError, match="status -3"):
            ctx.fill_groups("jc", [[0, 1]])
        assert ctx.shard_pairs() == pairs < n * (n - 1) // 2
    finally:
        ctx.set_shard(0, 1)
    # after all the refusals: still filling correctly, tie rule untouched
    assert ctx.tie_rule() == 5
    assert np.array_equal(ctx.fill_groups("aai", [[1, 2, 7], [0, n - 1]])[0], condensed_of(whole_aai, [1, 2, 7]))
    assert np.array_equal(square(ctx.fill("aai"), n, True), whole_aai) and ctx.shard_pairs() == n * (n - 1) // 2
    ctx.set_tie_rule(0)
    # aai before the residues are on the device
    ctx.upload(small_packed, residues=False)
    assert lib.pc_fill_groups(h, 4, 1, m_p, o_p, 1, out_p, None) == -3
    assert lib.pc_fill_groups(h, 1, 1, m_p, o_p, 1, out_p, None) == 0 and np.array_equal(out, condensed_of(whole_jc, [1, 2, 7]))
    # before any upload
    fresh = hip.Context(ctx.device_id)
    try:
        assert fresh._lib.pc_fill_groups(fresh._h, 1, 1, m_p, o_p, 1, out_p, None) == -3
    finally:
        fresh.close()


def test_an_empty_translation_is_refused_as_by_the_whole_fill(ctx, small_packed):
    """PC_ERR_DATA, as a whole fill: an empty translation in a shared pham cannot be aligned (the reference fails on it too), so aai /
    peq / aai_ppos are refused with the library's data status (-5); the set metrics never read a residue and still give the whole
    fill's value; the context fills correctly afterwards."""
    from phamclust_amd import hip
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    empty, other, third = Genome("e1"), Genome("e2"), Genome("e3")
    empty.add("p1", "")
    other.add("p1", "MK")
    third.add("p1", "MKV"); third.add("p2", "MA")
    ctx.upload(pack_genomes([empty, other, third]))
    for metric in ("aai", "peq", "aai_ppos"):
        with pytest.raises(hip.HipLibraryError, match="status -5"):
            ctx.fill_groups(metric, [[0, 1]])
        with pytest.raises(hip.HipLibraryError, match="status -5"):
            ctx.fill_groups(metric, [[1, 2], [0, 2]])
    with pytest.raises(hip.HipLibraryError):
        ctx.fill("aai")                                                                   # the whole fill refuses the same upload
    for metric in ("af", "jc"):
        whole = square(ctx.fill(metric, as_distance=False), 3, False)
        got = ctx.fill_groups(metric, [[0, 1], [0, 1, 2]], as_distance=False)
        assert np.array_equal(got[0], condensed_of(whole, [0, 1])) and np.array_equal(got[1], condensed_of(whole, [0, 1, 2]))
    assert ctx.fill_groups("af", [[0, 1]], as_distance=False)[0][0] == 1.0
    # a later correct fill works
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    whole = square(ctx.fill("peq"), n, True)
    assert np.array_equal(ctx.fill_groups("peq", [[1, 2, 7], [0, n - 1]])[0], condensed_of(whole, [1, 2, 7]))


def test_fill_groups_dev_leaves_the_vector_in_hbm(ctx, small_packed):
    import torch
    n = small_packed.n_genomes
    ctx.upload(small_packed)
    whole = square(ctx.fill("peq"), n, True)
    groups = [[0, 3, 9, 22], [], [4, 5], [1, 3, 9]]
    total = sum(len(g) * (len(g) - 1) // 2 for g in groups)
    out = torch.full((total + 1,), -1.0, dtype=torch.float64, device=f"cuda:{ctx.device_id}")
    st = ctx.fill_groups_dev("peq", True, groups, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert st["n_pairs"] == total and host[-1] == -1.0
    assert np.array_equal(host[:total], np.concatenate([condensed_of(whole, g) for g in groups]))


# ---- submatrices_de_novo, hierarchical_clustering_de_novo, the CLI ----------------------------------------------------------
def test_submatrices_de_novo_equals_extract_submatrix(small_genomes):
    from phamclust_amd import cli, matrix as M
    names = [g.name for g in small_genomes]
    n = len(names)
    groups = [names[3:9], [names[n - 1]], [names[k] for k in (20, 2, 11)], [1, 4, 5, 17], names[5:12]]   # names or indices, any order, overlapping
    for metric in ALL_METRICS:
        func = cli.METRICS[metric]
        for as_distance in (True, False):
            whole = M.matrix_de_novo(small_genomes, func, 1, as_distance=as_distance)
            uploads = []
            original = M.get_context().upload
            try:
                M.get_context().upload = lambda *a, **k: (uploads.append(1), original(*a, **k))[1]
                parts = M.submatrices_de_novo(small_genomes, func, groups, as_distance=as_distance)
            finally:
                del M.get_context().upload
            assert len(uploads) == 1 and len(parts) == len(groups)
            for group, part in zip(groups, parts):
                want_nodes = sorted(names[g] if isinstance(g, int) else g for g in group)          # genome-list order (the list is name-sorted)
                want = whole.extract_submatrix(want_nodes)
                assert part.nodes == want_nodes and part.is_distance == as_distance
                assert np.array_equal(part.to_ndarray(), want.to_ndarray()), (metric, as_distance, group)
    assert M.LAST_FILL["metric"] == "peq" and M.LAST_FILL["groups"] == len(groups)


def test_hierarchical_clustering_de_novo_uploads_once(monkeypatch, small_genomes):
    from phamclust_amd import cli, hip, matrix as M
    from phamclust_amd.clustering import hierarchical_clustering, hierarchical_clustering_de_novo
    calls = {"upload": 0, "fill_groups": 0, "fill_components": 0, "fill": 0}
    for name in calls:
        def counted(self, *args, _name=name, _inner=getattr(hip.Context, name), **kwargs):
            calls[_name] += 1
            return _inner(self, *args, **kwargs)
        monkeypatch.setattr(hip.Context, name, counted)
    for metric in ("jc", "peq"):
        func = cli.METRICS[metric]
        for linkage, eps in (("single", 0.75), ("average", 0.75), ("complete", 0.4)):
            for key in calls:
                calls[key] = 0
            got = hierarchical_clustering_de_novo(small_genomes, func, linkage, eps=eps)
            assert calls == {"upload": 1, "fill_groups": 1, "fill_components": 1, "fill": 0}, (metric, linkage, calls)
            assert M.LAST_FILL["metric"] == metric and M.LAST_FILL["groups"] >= 1 and M.LAST_FILL["n_components"] > 1 and M.LAST_FILL["n_pairs"] > 0
            want = hierarchical_clustering(M.matrix_de_novo(small_genomes, func, 1), linkage, eps=eps)
            assert [p.nodes for p in got] == [p.nodes for p in want]
            for a, b in zip(got, want):
                assert np.array_equal(a.to_ndarray(), b.to_ndarray())
            assert 1 < len(got) < len(small_genomes)


def _tree(root):
    return {p.relative_to(root).as_posix(): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file() and p.suffix != ".log"}


def _square_edges(text):
    """A squareform .tsv as a {pair: value text} map (tests/test_pipeline.py's rule: node order inside a cluster is no property of
    the reference, clustering.py:41-47 collects members in sets)."""
    lines = text.splitlines()
    names = lines[0].split("\t")[1:]
    assert [l.split("\t")[0] for l in lines[1:]] == names
    return {frozenset((l.split("\t")[0], b)): v for l in lines[1:] for b, v in zip(names, l.split("\t")[1:])}


def compare_cluster_directories(out, fixture):
    """The cluster_* and singletons directories of ``out`` against the reference's tree under tests/test_pipeline.py's rules: the
    same files; matrices as {pair: value} maps; the sub-clusters of a cluster as a partition (numbering among equal sizes is
    arbitrary)."""
    clustered = lambda rel: rel.startswith(("cluster_", "singletons/")) and not rel.endswith((".svg", ".html"))      # noqa: E731
    got = {p.relative_to(out).as_posix(): p for p in sorted(out.rglob("*")) if p.is_file()}
    want = {rel: text for rel, text in fixture["files"].items() if clustered(rel)}
    assert sorted(rel for rel in got if clustered(rel)) == sorted(want) and len(want) > 20
    parts_got, parts_want = {}, {}
    for rel, text in want.items():
        if text is None:
            continue
        if "/subcluster_" in rel:
            parts_want.setdefault(rel.split("/")[0], []).append(_square_edges(text))
            parts_got.setdefault(rel.split("/")[0], []).append(_square_edges(got[rel].read_text()))
        else:
            assert _square_edges(got[rel].read_text()) == _square_edges(text), rel
    assert parts_want
    for cluster in parts_want:
        key = lambda e: sorted(sorted(k) for k in e)          # noqa: E731
        assert sorted(map(key, parts_got[cluster])) == sorted(map(key, parts_want[cluster])), cluster


@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_cli_no_matrix_reproduces_a_dense_run(tmp_path, metric):
    from phamclust_amd.scripts.phamclust import main
    tsv = os.path.join(REPO, "tests", "golden", "small_input.tsv")
    fixture = json.load(open(os.path.join(REPO, "tests", "golden", "pipeline_jc", "tree.json")))

    def run(name, *extra):
        out = tmp_path / name
        main([tsv, str(out), "-m", metric, "-k", str(fixture["k_min"]), "-t", "1", *extra])
        return out
    dense, sparse, adjacency = run("dense"), run("no_matrix", "--no-matrix"), run("adjacency", "--adjacency-only")
    a, b = _tree(dense), _tree(sparse)
    clustered = [rel for rel in a if rel.startswith(("cluster_", "singletons/"))]
    assert len(clustered) > 20 and any("subcluster_" in rel for rel in clustered) and any(rel.startswith("singletons/") for rel in clustered)
    assert sorted(rel for rel in b if rel.startswith(("cluster_", "singletons/"))) == sorted(clustered)
    # byte for byte, but for the heatmap renderings: plotly writes random element ids into every .svg / .html (their presence is held above)
    assert [rel for rel in clustered if a[rel] != b[rel] and not rel.endswith((".svg", ".html"))] == []
    assert sorted(rel for rel in b if rel not in a) == []
    assert sorted(rel for rel in a if rel not in b) == sorted([f"{fixture['md5_tmp_dir']}/02_distmats/{metric}_distance_matrix.tsv", f"{metric}_heatmap.html",
                                                                f"{metric}_heatmap.svg", f"pairwise_{metric}_similarities.tsv"])
    assert not list(sparse.rglob("*_similarities.tsv")) and not list(sparse.rglob("*distance_matrix.tsv")) and not list(sparse.rglob("02_distmats"))
    assert (sparse / f"pairwise_{metric}_adjacency.tsv").read_bytes() == (adjacency / f"pairwise_{metric}_adjacency.tsv").read_bytes()
    log = (sparse / "phamclust.log").read_text()
    assert "--no-matrix" in log and f"pairwise_{metric}_similarities.tsv" in log and "are not written" in log
    if metric == "jc":                                              # the reference's own tree, under that file's comparison rules
        compare_cluster_directories(sparse, fixture)
