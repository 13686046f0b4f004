"""The between-groups fill (pc_fill_between / Context.fill_between / MultiContext.fill_between / between_de_novo / --cluster-table) on
the GPU (run with ``-m gpu``).

The expected table always comes from a DENSE vector -- a golden file the live reference wrote, or (hand-built collections) the same
context's whole fill, which the rest of the suite pins -- through ``GroupLinkage.from_dense``, the host statement that
tests/test_between_host.py holds to brute force.  Every comparison is exact: ``np.array_equal`` on the four integer arrays.  An
element taken twice or dropped at a row's odd start, at a segment seam or at a slab seam shows in ``count``; an accumulator that does
not survive from slab to slab, a sum that loses its upper 32 bits, an extreme taken over the wrong group or a merge that counts a
stretch twice fails here; so does a walk that leaves the context sharded."""

import ctypes
import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN, golden_file, read_lower_triangle, synth200_file
from test_between_host import EMPTY, partitions
from test_gpu_components import hand_built

pytestmark = pytest.mark.gpu

MILLION = 1000000


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


@pytest.fixture(scope="module")
def multis(native_built):
    """MultiContext([0] * world), made on first use and kept for the module."""
    from phamclust_amd import hip
    made = {}

    def get(world):
        if world not in made:
            made[world] = hip.MultiContext([0] * world)
        return made[world]
    yield get
    for multi in made.values():
        multi.close()


_GOLDEN = {}


def golden_matrix(name, metric):
    """The dense distance matrix of a fixture, its names g0 .. in fill order, once per (fixture, metric)."""
    from phamclust_amd.matrix import SymMatrix
    if (name, metric) not in _GOLDEN:
        names, condensed, _ = read_lower_triangle(golden_file(metric) if name == "small" else synth200_file(metric))
        _GOLDEN[name, metric] = SymMatrix.from_condensed(names, condensed, is_distance=True)
    return _GOLDEN[name, metric]


def labels_of(names, groups):
    at = {name: k for k, name in enumerate(names)}
    label = np.full(len(names), -1, dtype=np.int32)
    for a, group in enumerate(groups):
        label[[at[name] for name in group]] = a
    assert (label >= 0).all()
    return label


def check(got, want, label, sizes=None):
    """The four arrays of a fill against a GroupLinkage: dtype, shape, symmetry, values; with ``sizes`` the counts by arithmetic."""
    total, count, lo, hi = got
    g = len(want)
    assert total.dtype == count.dtype == np.int64 and lo.dtype == hi.dtype == np.int32, label
    for arr, ref in ((total, want.sum), (count, want.cnt), (lo, want.lo), (hi, want.hi)):
        assert arr.shape == (g, g) and np.array_equal(arr, arr.T), label
        assert np.array_equal(arr, ref), label
    if sizes is not None:
        sizes = np.asarray(sizes, dtype=np.int64)
        expect = np.outer(sizes, sizes)
        np.fill_diagonal(expect, sizes * (sizes - 1) // 2)
        assert np.array_equal(count, expect), label
    empty = count == 0
    assert (total[empty] == 0).all() and (lo[empty] == EMPTY[2]).all() and (hi[empty] == EMPTY[3]).all(), label


# ---- 1: the fixtures the live reference wrote --------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_table_equals_the_dense_fixture(ctx, small_packed, synth200_packed, name, metric):
    """Distances against the golden file; the similarity table against the golden matrix inverted, and against inverted() of the
    distance fill's table."""
    from phamclust_amd.matrix import GroupLinkage
    packed = small_packed if name == "small" else synth200_packed
    matrix = golden_matrix(name, metric)
    names = matrix.nodes
    similar = matrix.extract_submatrix(names).invert()
    ctx.upload(packed)
    for tag, groups in partitions(matrix).items():
        label = labels_of(names, groups)
        sizes = [len(group) for group in groups]
        *got, st = ctx.fill_between(metric, label, as_distance=True, want_stats=True)
        check(got, GroupLinkage.from_dense(matrix, groups), (name, metric, tag, "distance"), sizes)
        assert st["n_groups"] == len(groups) and st["n_slabs"] == 1 and st["n_pairs"] == len(names) * (len(names) - 1) // 2, (name, metric, tag)
        assert st["ms_reduce"] > 0.0 and st["ms_finish"] > 0.0, (name, metric, tag)
        distance = GroupLinkage(groups, *got, is_distance=True)
        got = ctx.fill_between(metric, label, len(groups), as_distance=False)
        check(got, distance.inverted(), (name, metric, tag, "similarity: the distance fill inverted"), sizes)
        check(got, GroupLinkage.from_dense(similar, groups), (name, metric, tag, "similarity: the inverted matrix"), sizes)


def test_similarity_table_at_a_decimal_tie(ctx, synth200_packed):
    """Pair (36, 115) of synth200 has an af similarity at a decimal tie: the similarity FILL delivers 0.013688 where the distance fill
    delivers 0.986313, both rounded up (the oracle gives the same two values).  The similarity table holds the distance's complement,
    986,313 -> 13,687, as ``SymMatrix.invert`` does, not the similarity fill's 13,688."""
    n = synth200_packed.n_genomes
    ctx.upload(synth200_packed, residues=False)
    at = 36 * n - 36 * 37 // 2 + (115 - 36 - 1)
    assert (float(ctx.fill("af", as_distance=True)[at]), float(ctx.fill("af", as_distance=False)[at])) == (0.986313, 0.013688)
    label = np.zeros(n, dtype=np.int32)
    label[36], label[115] = 1, 2
    for slab_bytes in (0, 8 * 199):
        _, count, lo, hi = ctx.fill_between("af", label, 3, as_distance=True, slab_bytes=slab_bytes)
        assert (int(count[1, 2]), int(lo[1, 2]), int(hi[1, 2])) == (1, 986313, 986313)
        total, count, lo, hi = ctx.fill_between("af", label, 3, as_distance=False, slab_bytes=slab_bytes)
        assert (int(total[1, 2]), int(count[1, 2]), int(lo[1, 2]), int(hi[1, 2])) == (13687, 1, 13687, 13687)


# ---- 2: the slab cut ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_the_result_does_not_depend_on_the_slab_cut(ctx, synth200_packed, metric):
    from phamclust_amd.hip import Context
    from phamclust_amd.matrix import GroupLinkage
    matrix = golden_matrix("synth200", metric)
    n = len(matrix)
    parts = partitions(matrix)
    ctx.upload(synth200_packed)
    for tag in ("mod7", "cc_mid"):
        groups = parts[tag]
        want = GroupLinkage.from_dense(matrix, groups)
        label = labels_of(matrix.nodes, groups)
        for slab_bytes in (8 * 64, 8 * 199, 8 * 1000):
            *got, st = ctx.fill_between(metric, label, slab_bytes=slab_bytes, want_stats=True)
            check(got, want, (metric, tag, slab_bytes), [len(group) for group in groups])
            assert st["n_slabs"] == len(Context.chunk_plan(np.arange(n, dtype=np.uint64), slab_bytes // 8)) - 1 == len(Context.edge_slabs(n, slab_bytes)) - 1
            assert st["n_slabs"] > 10, (metric, tag, slab_bytes)
            assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride(), (metric, tag, slab_bytes)
    assert np.array_equal(ctx.fill(metric), matrix.to_ndarray(condensed=True))


# ---- 3: row shapes -----------------------------------------------------------------------------------
def whole_fill_table(ctx, metric, n, label, n_groups, as_distance=True):
    """``GroupLinkage.from_dense`` of the same context's whole distance fill under the labels; a similarity table: of that matrix inverted."""
    from phamclust_amd.matrix import GroupLinkage, SymMatrix
    names = [f"n{k:05d}" for k in range(n)]
    condensed = ctx.fill(metric, as_distance=True) if n > 1 else np.empty(0)
    matrix = SymMatrix.from_condensed(names, condensed, is_distance=True)
    if not as_distance:
        matrix.invert()
    return GroupLinkage.from_dense(matrix, [[names[g] for g in np.flatnonzero(np.asarray(label) == a).tolist()] for a in range(n_groups)])


def test_two_and_three_genomes(ctx):
    """Rows of length 0, 1 and 2; lbase 0, 0, 1 (an odd row start); every way to label them."""
    for n in (2, 3):
        for kind in ("identical", "chain"):
            ctx.upload(hand_built(n, kind))
            for metric in ("jc", "peq"):
                for label in ([0] * n, list(range(n)), [1, 0, 1][:n], [0, 2, 2][:n]):
                    g = max(label) + 1
                    for as_distance in (True, False):
                        want = whole_fill_table(ctx, metric, n, label, g, as_distance)
                        for slab_bytes in (0, 8):
                            got = ctx.fill_between(metric, label, g, as_distance=as_distance, slab_bytes=slab_bytes)
                            check(got, want, (n, kind, metric, label, as_distance, slab_bytes), np.bincount(label, minlength=g))


@pytest.mark.parametrize("kind", ["identical", "disjoint"])
def test_one_group_of_equal_values(ctx, kind):
    """130 genomes in one group: 8,385 pairs, all 0 (identical) or all 10^6 (disjoint) on distances -- the latter a sum of 8.4 * 10^9,
    which needs its upper 32 bits -- through the wave's one-group reduction."""
    n = 130
    pairs = n * (n - 1) // 2
    ctx.upload(hand_built(n, kind))
    value = 0 if kind == "identical" else MILLION
    for metric in ("jc", "peq"):
        for as_distance in (True, False):
            micro = value if as_distance else MILLION - value
            for slab_bytes in (0, 8 * 100):
                total, count, lo, hi = ctx.fill_between(metric, np.zeros(n, dtype=np.int32), 1, as_distance=as_distance, slab_bytes=slab_bytes)
                assert (total.tolist(), count.tolist(), lo.tolist(), hi.tolist()) == ([[pairs * micro]], [[pairs]], [[micro]], [[micro]]), (kind, metric, as_distance)
    assert pairs * MILLION > 2 ** 32
    label = np.arange(n, dtype=np.int32) % 2                               # and two interleaved groups: no wave is of one group
    check(ctx.fill_between("jc", label, 2), whole_fill_table(ctx, "jc", n, label, 2), (kind, "two groups"), [65, 65])


def test_chain_every_entry_one_pair_and_two_groups(ctx):
    n = 129
    ctx.upload(hand_built(n, "chain"))
    for metric in ("jc", "peq"):
        label = np.arange(n, dtype=np.int32)
        want = whole_fill_table(ctx, metric, n, label, n)
        for slab_bytes in (0, 8 * 129):
            got = ctx.fill_between(metric, label, n, slab_bytes=slab_bytes)
            check(got, want, (metric, "G = 129", slab_bytes), np.ones(n))
            off = ~np.eye(n, dtype=bool)                                   # (the diagonal: one-genome groups, empty)
            assert np.array_equal(got[2][off], got[3][off]) and (got[1] == 1 - np.eye(n, dtype=np.int64)).all()
        label = (np.arange(n) >= 40).astype(np.int32)
        check(ctx.fill_between(metric, label, 2), whole_fill_table(ctx, metric, n, label, 2), (metric, "G = 2"), [40, 89])


def test_rows_longer_than_two_segments(ctx):
    """A chain of 2 * segment + 3 genomes under jc with g % 5 labels, against the same context's whole fill: the last rows take three
    workgroups each, the third an odd tail of a few elements; a slab cut on top moves the rows' starts."""
    from phamclust_amd.hip import Context
    segment = Context.between_segment()
    if segment == 0:
        pytest.skip("rows are never split")
    n = 2 * segment + 3
    ctx.upload(hand_built(n, "chain"), residues=False)
    label = np.arange(n, dtype=np.int32) % 5
    want = whole_fill_table(ctx, "jc", n, label, 5)
    sizes = np.bincount(label, minlength=5)
    check(ctx.fill_between("jc", label, 5), want, "one slab", sizes)
    *got, st = ctx.fill_between("jc", label, 5, slab_bytes=8 * 3 * n, want_stats=True)
    check(got, want, "slabs of three rows", sizes)
    assert st["n_slabs"] > 1000


# ---- 4: limits ---------------------------------------------------------------------------------------
def test_limits(ctx, synth200_packed):
    from phamclust_amd.hip import Context, HipLibraryError
    from phamclust_amd.matrix import GroupLinkage
    from phamclust_amd.pack import pack_genomes
    matrix = golden_matrix("synth200", "jc")
    names = matrix.nodes
    n = len(names)
    ctx.upload(synth200_packed, residues=False)
    top = Context.BETWEEN_MAX_GROUPS
    label = np.arange(n, dtype=np.int32) % top                             # = g: most groups are empty
    got = ctx.fill_between("jc", label, top)
    want = GroupLinkage.from_dense(matrix, [[names[g]] if g < n else [] for g in range(top)])
    check(got, want, "G at the limit", np.bincount(label, minlength=top))
    assert (got[1][n:, :] == 0).all() and (got[2][n:, :] == EMPTY[2]).all() and (got[3][:, n:] == EMPTY[3]).all()
    high = np.zeros(n, dtype=np.int32)
    high[7], high[n - 1] = top - 1, top - 2                                # the last rows of the table, reached from both sides
    check(ctx.fill_between("jc", high, top), GroupLinkage.from_dense(matrix, [[x for g, x in enumerate(names) if high[g] == a] for a in range(top)]),
          "the table's last rows")
    with pytest.raises(HipLibraryError, match=rf"status -4.*{top + 1}.*{top}"):
        ctx.fill_between("jc", label, top + 1)
    with pytest.raises(HipLibraryError, match="status -1.*genome 3 has label 5"):
        ctx.fill_between("jc", [0, 1, 2, 5] + [0] * (n - 4), 5)
    with pytest.raises(HipLibraryError, match="status -1.*genome 0 has label -1"):
        ctx.fill_between("jc", [-1] + [0] * (n - 1), 1)
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_between("jc", label, 0)
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_between("jc", np.zeros(n, dtype=np.int32), 1, slab_bytes=-8)
    # by code, through the C-ABI: NULL group, a missing output pointer, peq before the residues; every output nulled
    from phamclust_amd.hip import _i32p, _i64p
    lib, h = ctx._lib, ctx._h
    zeros = np.zeros(n, dtype=np.int32)

    def call(metric, group=zeros, n_groups=1, with_lo=True):
        ps, pc, pl, ph, ns = _i64p(), _i64p(), _i32p(), _i32p(), ctypes.c_int32(7)
        rc = lib.pc_fill_between(h, metric, 1, group.ctypes.data_as(_i32p) if group is not None else None, n_groups, 0, ctypes.byref(ps),
                                 ctypes.byref(pc), ctypes.byref(pl) if with_lo else None, ctypes.byref(ph), ctypes.byref(ns), None)
        return rc, bool(ps), bool(pc), bool(pl), bool(ph), ns.value

    refused = (False, False, False, False, 0)
    assert call(1, group=None) == (-1,) + refused
    assert call(1, with_lo=False) == (-1,) + refused
    assert call(5) == (-3,) + refused
    assert call(9) == (-1,) + refused
    assert call(1, n_groups=top + 1) == (-4,) + refused
    assert call(1) == (0, True, True, True, True, 1)
    a, b = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.pc_last_between_times(h, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0      # no stats asked
    ctx.set_shard(1, 3)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):
            ctx.fill_between("jc", zeros, 1)
    finally:
        ctx.set_shard(0, 1)
    # a loan ends with the next fill
    lent = ctx.fill_between("jc", zeros, 1, borrow=True)
    assert int(np.asarray(lent[1])[0, 0]) == n * (n - 1) // 2
    ctx.fill("jc")
    with pytest.raises(HipLibraryError):
        np.asarray(lent[0])
    # one genome: nothing runs on the device, every entry empty; no genome: nothing to upload at all
    ctx.upload(hand_built(1, "identical"))
    for g in (1, 3):
        *got, st = ctx.fill_between("peq", [0], g, want_stats=True)
        assert [arr.tolist() for arr in got] == [[[v] * g] * g for v in (EMPTY[1], EMPTY[0], EMPTY[2], EMPTY[3])] and st["n_slabs"] == 0
    with pytest.raises(ValueError):
        pack_genomes([])


# ---- 5: several devices ------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_several_devices_equal_the_single_context(ctx, multis, synth200_packed, metric, world):
    from phamclust_amd.hip import MultiContext
    from test_gpu_multi_slabs import check_route, costs
    matrix = golden_matrix("synth200", metric)
    n = len(matrix)
    parts = partitions(matrix)
    ctx.upload(synth200_packed)
    multi = multis(world)
    multi.upload(synth200_packed, residues=False)                           # the residues follow on demand, on every device
    bounds = MultiContext.slab_stretches(costs(ctx, synth200_packed, metric), world).tolist()
    for tag in ("mod7", "cc_mid"):
        label = labels_of(matrix.nodes, parts[tag])
        for as_distance in (True, False):
            want = ctx.fill_between(metric, label, as_distance=as_distance)
            for slab_bytes in (0, 8 * 4000):
                *got, st = multi.fill_between(metric, label, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
                for a, b in zip(got, want):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (metric, world, tag, as_distance, slab_bytes)
                assert st["n_groups"] == len(parts[tag])
                check_route(st, world, bounds, n, slab_bytes, (metric, world, tag, as_distance, slab_bytes))


def test_fewer_genomes_than_devices(ctx, multis):
    """Three genomes on four devices: at least one stretch is empty, its device launches and ships nothing; one genome: the root alone."""
    multi = multis(4)
    packed = hand_built(3, "chain")
    ctx.upload(packed)
    multi.upload(packed)
    for metric in ("jc", "peq"):
        for label in ([0, 0, 0], [0, 1, 2], [1, 0, 1]):
            want = ctx.fill_between(metric, label, 3)
            *got, st = multi.fill_between(metric, label, 3, slab_bytes=8, want_stats=True)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (metric, label)
            assert st["stretches"][0] == 0 and st["stretches"][-1] == 3 and any(a == b for a, b in zip(st["stretches"], st["stretches"][1:]))
            assert st["n_pairs"] == 3
    multi.upload(hand_built(1, "chain"))
    got = multi.fill_between("jc", [0], 2)
    assert [arr.tolist() for arr in got] == [[[v] * 2] * 2 for v in (EMPTY[1], EMPTY[0], EMPTY[2], EMPTY[3])]


# ---- 6: above the C-ABI ------------------------------------------------------------------------------
def test_between_de_novo(small_genomes, native_built):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    names = [g.name for g in small_genomes]
    dense = golden_matrix("small", "jc")
    assert dense.nodes == names
    groups = [names[r::4] for r in range(4)]
    found = M.between_de_novo(small_genomes, cli.METRICS["jc"], groups)
    assert found == M.GroupLinkage.from_dense(dense, groups) and M.LAST_FILL["metric"] == "jc" and M.LAST_FILL["n_slabs"] == 1
    by_index = M.between_de_novo(small_genomes, cli.METRICS["jc"], [list(range(r, len(names), 4)) for r in range(4)], as_distance=False, slab_bytes=8 * 40)
    assert by_index == found.inverted() and M.LAST_FILL["n_slabs"] > 1


def test_cluster_table_run(tmp_path, small_genomes, native_built, monkeypatch):
    """--cluster-table on the dense route and on --no-matrix: the three files, byte for byte the same on both routes, the square the
    host statement's over the final clusters; and everything else the run writes is what it writes without the flag."""
    from phamclust_amd.matrix import GroupLinkage, read_squareform
    from phamclust_amd.scripts.phamclust import main
    monkeypatch.setenv("PHAMCLUST_NO_HEATMAPS", "1")
    infile = os.path.join(GOLDEN, "small_input.tsv")
    new = ["cluster_jc_similarities.tsv", "cluster_table_jc.tsv"]

    def run(tag, *flags):
        out = tmp_path / tag
        main([infile, str(out), "-m", "jc"] + list(flags))
        return out, {p.relative_to(out).as_posix(): p.read_bytes() for p in out.rglob("*") if p.is_file() and p.suffix != ".log"}

    plain_out, plain = run("plain")
    dense_out, dense = run("dense", "--cluster-table")
    bare_out, bare = run("bare", "--no-matrix")
    sparse_out, sparse = run("sparse", "--no-matrix", "--cluster-table")
    assert sorted(set(dense) - set(plain)) == new == sorted(set(sparse) - set(bare))
    assert {k: v for k, v in dense.items() if k not in new} == plain and {k: v for k, v in sparse.items() if k not in new} == bare
    for name in new:
        assert dense[name] == sparse[name] and len(dense[name]) > 0, name
    assert "cluster table (between-groups fill)" in (dense_out / "phamclust.log").read_text()
    # the square is the host statement's over the final clusters: cluster_1 .. cluster_k, then the singletons
    clusters = sorted((p for p in dense_out.iterdir() if p.is_dir() and p.name.startswith("cluster_")), key=lambda p: int(p.name.split("_")[1]))
    groups = [sorted(f.stem for f in (c / "genomes").iterdir()) for c in clusters]
    single = dense_out / "singletons" / "genomes"
    rows = list(read_squareform(dense_out / "cluster_jc_similarities.tsv"))
    group_names = [row[0] for row in rows]
    assert group_names[:len(clusters)] == [c.name for c in clusters]
    lone = group_names[len(clusters):]
    assert sorted(lone) == (sorted(f.stem for f in single.iterdir()) if single.is_dir() else [])
    groups += [[name] for name in lone]
    assert sorted(x for group in groups for x in group) == [g.name for g in small_genomes] and len(groups) > 1
    want = GroupLinkage.from_dense(golden_matrix("small", "jc"), groups).inverted()
    assert np.array_equal(np.array([row[1] for row in rows]), want.to_symmatrix(group_names, "mean").to_ndarray())
    from phamclust_amd.matrix import between_from_file
    names_back, table = between_from_file(dense_out / "cluster_table_jc.tsv", groups=groups, is_distance=False)
    assert names_back == group_names and table == want


def test_timing_tool_writes_its_lines(tmp_path, native_built):
    import subprocess
    import sys
    out = tmp_path / "between_fill.txt"
    tool = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "between_timing.py")
    done = subprocess.run([sys.executable, tool, "--n", "300", "--n-peq", "120", "--repeats", "2", "--warmup", "1", "--out", str(out)],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    text = out.read_text()
    for workload in ("jc components", "peq components", "jc one group", "jc 2048 round-robin"):
        assert workload in text, text
    assert text.count("between: pass") == 4 and text.count("dense route: fill+D2H") == 4 and "ratio" in text
