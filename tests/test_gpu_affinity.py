"""The affinity fill (pc_fill_affinity / Context.fill_affinity / MultiContext.fill_affinity / affinity_de_novo / --cluster-fit) on the
GPU (run with ``-m gpu``).

The expected result always comes from a DENSE vector -- a golden file the live reference wrote, or (hand-built collections) the same
context's whole fill, which the rest of the suite pins -- through ``GroupAffinity.from_dense``, the host statement that
tests/test_affinity_host.py holds to brute force.  Every comparison is exact: ``np.array_equal`` on integer arrays.  An element taken
twice or dropped in either pass shows in a sum; a table that does not survive from slab to slab, a sum that loses its upper 32 bits, a
column pass that misses a group's members at a slab seam or a source block's ragged end, a finish that breaks a tie the wrong way or a
merge that counts a stretch twice fails here; so does a walk that leaves the context sharded."""

import ctypes
import os

import numpy as np
import pytest

from conftest import ALL_METRICS, GOLDEN
from test_affinity_host import EMPTY_ENTRY
from test_between_host import partitions
from test_gpu_between import golden_matrix, labels_of
from test_gpu_components import hand_built

pytestmark = pytest.mark.gpu

MILLION = 1000000
ARRAYS = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")


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


def check(got, want, label, table=True):
    """The dict of a fill against a GroupAffinity: dtype, shape and value of every array; the table when it was asked for."""
    n, g = len(want.nodes), len(want.groups)
    for name in ARRAYS:
        arr, ref = got[name], getattr(want, name)
        assert arr.dtype == ref.dtype and arr.shape == ((3, n) if name == "near_group" else (n,)), (label, name)
        assert np.array_equal(arr, ref), (label, name)
    if not table:
        assert got["table"] is None, label
        return
    for arr, ref, dtype in zip(got["table"], want.table, (np.int64, np.int32, np.int32)):
        assert arr.dtype == dtype and arr.shape == (n, g) and np.array_equal(arr, ref), label


def same(a, b, label):
    for name in ARRAYS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (label, name)
    assert (a["table"] is None) == (b["table"] is None), label
    if a["table"] is not None:
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a["table"], b["table"])), label


# ---- 1: the fixtures the live reference wrote --------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
@pytest.mark.parametrize("name", ["small", "synth200"])
def test_affinity_equals_the_dense_fixture(ctx, small_packed, synth200_packed, name, metric):
    """Distances against the golden file; similarities against the golden matrix inverted and against inverted() of the distance fill;
    with and without the table the O(N) arrays are the same."""
    from phamclust_amd.matrix import GroupAffinity
    packed = small_packed if name == "small" else synth200_packed
    matrix = golden_matrix(name, metric)
    names = matrix.nodes
    similar = matrix.extract_submatrix(names).invert()
    ctx.upload(packed)
    for tag, groups in partitions(matrix).items():
        label = labels_of(names, groups)
        want = GroupAffinity.from_dense(matrix, groups)
        got = ctx.fill_affinity(metric, label, as_distance=True, want_table=True, want_stats=True)
        st = got.pop("stats")
        check(got, want, (name, metric, tag, "distance"))
        assert st["n_groups"] == len(groups) and st["n_slabs"] == 1 and st["n_pairs"] == len(names) * (len(names) - 1) // 2, (name, metric, tag)
        assert st["ms_rows"] > 0.0 and st["ms_cols"] > 0.0 and st["ms_finish"] > 0.0, (name, metric, tag)
        check(ctx.fill_affinity(metric, label, len(groups)), want, (name, metric, tag, "distance, no table"), table=False)
        got = ctx.fill_affinity(metric, label, len(groups), as_distance=False, want_table=True)
        check(got, want.inverted(), (name, metric, tag, "similarity: the distance statement inverted"))
        check(got, GroupAffinity.from_dense(similar, groups), (name, metric, tag, "similarity: the inverted matrix"))
        check(ctx.fill_affinity(metric, label, len(groups), as_distance=False), want.inverted(), (name, metric, tag, "similarity, no table"), table=False)


def test_similarity_table_at_a_decimal_tie(ctx, synth200_packed):
    """Pair (36, 115) of synth200 has an af similarity at a decimal tie (tests/test_gpu_between.py): the similarity statement holds the
    distance's complement, 986,313 -> 13,687, as ``SymMatrix.invert`` does, not the similarity fill's 13,688."""
    n = synth200_packed.n_genomes
    ctx.upload(synth200_packed, residues=False)
    label = np.zeros(n, dtype=np.int32)
    label[36], label[115] = 1, 2
    for slab_bytes in (0, 8 * 199):
        got = ctx.fill_affinity("af", label, 3, as_distance=True, want_table=True, slab_bytes=slab_bytes)
        assert [int(arr[36, 2]) for arr in got["table"]] == [986313] * 3 == [int(arr[115, 1]) for arr in got["table"]]
        got = ctx.fill_affinity("af", label, 3, as_distance=False, want_table=True, slab_bytes=slab_bytes)
        assert [int(arr[36, 2]) for arr in got["table"]] == [13687] * 3 == [int(arr[115, 1]) for arr in got["table"]]


# ---- 2: the slab cut ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "peq"])
def test_the_result_does_not_depend_on_the_slab_cut(ctx, synth200_packed, metric):
    from phamclust_amd.hip import Context
    from phamclust_amd.matrix import GroupAffinity
    matrix = golden_matrix("synth200", metric)
    n = len(matrix)
    parts = partitions(matrix)
    ctx.upload(synth200_packed)
    for tag in ("mod7", "cc_mid"):
        groups = parts[tag]
        want = GroupAffinity.from_dense(matrix, groups)
        label = labels_of(matrix.nodes, groups)
        for slab_bytes in (8 * 64, 8 * 199, 8 * 1000):
            got = ctx.fill_affinity(metric, label, slab_bytes=slab_bytes, want_table=True, want_stats=True)
            st = got.pop("stats")
            check(got, want, (metric, tag, slab_bytes))
            assert st["n_slabs"] == len(Context.edge_slabs(n, slab_bytes)) - 1 and st["n_slabs"] > 10, (metric, tag, slab_bytes)
            assert ctx.shard_pairs() == n * (n - 1) // 2 == ctx.shard_stride(), (metric, tag, slab_bytes)
    assert np.array_equal(ctx.fill(metric), matrix.to_ndarray(condensed=True))


# ---- 3: shapes where the passes can go wrong ---------------------------------------------------------
def whole_fill_affinity(ctx, metric, n, label, n_groups, as_distance=True):
    """``GroupAffinity.from_dense`` of the same context's whole distance fill under the labels; a similarity statement: of that matrix
    inverted."""
    from phamclust_amd.matrix import GroupAffinity, SymMatrix
    names = [f"n{k:05d}" for k in range(n)]
    condensed = ctx.fill(metric, as_distance=True) if n > 1 else np.empty(0)
    matrix = SymMatrix.from_condensed(names, condensed, is_distance=True)
    if not as_distance:
        matrix.invert()
    return GroupAffinity.from_dense(matrix, [[names[g] for g in np.flatnonzero(np.asarray(label) == a).tolist()] for a in range(n_groups)])


def test_two_and_three_genomes(ctx):
    """Rows of length 0, 1 and 2; lbase 0, 0, 1 (an odd row start); every way to label them."""
    for n in (2, 3):
        for kind in ("identical", "chain"):
            ctx.upload(hand_built(n, kind))
            for metric in ("jc", "peq"):
                for label in ([0] * n, list(range(n)), [1, 0, 1][:n], [0, 2, 2][:n]):
                    g = max(label) + 1
                    for as_distance in (True, False):
                        want = whole_fill_affinity(ctx, metric, n, label, g, as_distance)
                        for slab_bytes in (0, 8):
                            got = ctx.fill_affinity(metric, label, g, as_distance=as_distance, slab_bytes=slab_bytes, want_table=True)
                            check(got, want, (n, kind, metric, label, as_distance, slab_bytes))


@pytest.mark.parametrize("kind", ["identical", "disjoint"])
def test_one_group_of_equal_values(ctx, kind):
    """130 genomes in one group, all values 0 (identical) or all 10^6 (disjoint) on distances, through the row pass's one-group wave
    reduction; then two interleaved groups, where no wave is of one group."""
    n = 130
    ctx.upload(hand_built(n, kind))
    value = 0 if kind == "identical" else MILLION
    for metric in ("jc", "peq"):
        for as_distance in (True, False):
            micro = value if as_distance else MILLION - value
            for slab_bytes in (0, 8 * 100):
                got = ctx.fill_affinity(metric, np.zeros(n, dtype=np.int32), 1, as_distance=as_distance, slab_bytes=slab_bytes, want_table=True)
                assert got["own_sum"].tolist() == [(n - 1) * micro] * n and got["own_lo"].tolist() == got["own_hi"].tolist() == [micro] * n, (kind, metric)
                assert got["near_group"].tolist() == [[-1] * n] * 3 and got["near_sum"].tolist() == [0] * n, (kind, metric)
                assert got["near_lo"].tolist() == [EMPTY_ENTRY[1]] * n and got["near_hi"].tolist() == [-1] * n, (kind, metric)
                assert np.array_equal(got["table"][0][:, 0], got["own_sum"]), (kind, metric)
    label = np.arange(n, dtype=np.int32) % 2
    for slab_bytes in (0, 8 * 100):
        check(ctx.fill_affinity("jc", label, 2, want_table=True, slab_bytes=slab_bytes), whole_fill_affinity(ctx, "jc", n, label, 2), (kind, "two groups"))


def test_chain_every_entry_one_pair(ctx):
    n = 129
    ctx.upload(hand_built(n, "chain"))
    for metric in ("jc", "peq"):
        label = np.arange(n, dtype=np.int32)
        want = whole_fill_affinity(ctx, metric, n, label, n)
        for slab_bytes in (0, 8 * 129):
            got = ctx.fill_affinity(metric, label, n, slab_bytes=slab_bytes, want_table=True)
            check(got, want, (metric, "G = 129", slab_bytes))
            off = ~np.eye(n, dtype=bool)                                   # (the diagonal: one-genome groups, empty)
            assert np.array_equal(got["table"][1][off], got["table"][2][off]) and np.array_equal(got["table"][0][off], got["table"][1][off]), metric
        label = (np.arange(n) >= 40).astype(np.int32)
        check(ctx.fill_affinity(metric, label, 2, want_table=True), whole_fill_affinity(ctx, metric, n, label, 2), (metric, "G = 2"))


def test_source_block_edges_and_slab_seams(ctx):
    """N = block + 1 (a last source block of one lane) and 2 * block - 1 (a block whose rows all start inside it); labels g % 5 with
    slabs of three rows: every group's members straddle every slab seam."""
    from phamclust_amd.hip import Context
    block = Context.affinity_block()
    for n in (block + 1, 2 * block - 1):
        ctx.upload(hand_built(n, "chain"), residues=False)
        label = np.arange(n, dtype=np.int32) % 5
        want = whole_fill_affinity(ctx, "jc", n, label, 5)
        check(ctx.fill_affinity("jc", label, 5, want_table=True), want, (n, "one slab"))
        got = ctx.fill_affinity("jc", label, 5, want_table=True, slab_bytes=8 * 3 * n, want_stats=True)
        assert got.pop("stats")["n_slabs"] >= n // 6, n
        check(got, want, (n, "slabs of three rows"))
        check(ctx.fill_affinity("jc", np.zeros(n, dtype=np.int32), 1, want_table=True, slab_bytes=8 * 3 * n),
              whole_fill_affinity(ctx, "jc", n, np.zeros(n, dtype=np.int32), 1), (n, "one group, slabs of three rows"))


def test_sums_above_32_bits(ctx):
    """4,400 disjoint genomes in one group under jc: every own sum is 4,399 * 10^6 > 2^32, half of it from each pass."""
    n = 4400
    ctx.upload(hand_built(n, "disjoint"), residues=False)
    got = ctx.fill_affinity("jc", np.zeros(n, dtype=np.int32), 1)
    assert (n - 1) * MILLION > 2 ** 32
    assert (got["own_sum"] == (n - 1) * MILLION).all() and (got["own_lo"] == MILLION).all() and (got["own_hi"] == MILLION).all()
    assert (got["near_group"] == -1).all()
    got = ctx.fill_affinity("jc", np.zeros(n, dtype=np.int32), 1, as_distance=False, slab_bytes=8 * 1000000)
    assert (got["own_sum"] == 0).all() and (got["own_lo"] == 0).all() and (got["own_hi"] == 0).all()


# ---- 4: limits ---------------------------------------------------------------------------------------
def test_limits(ctx, synth200_packed):
    from phamclust_amd.hip import Context, HipLibraryError
    from phamclust_amd.matrix import GroupAffinity
    from phamclust_amd.pack import pack_genomes
    matrix = golden_matrix("synth200", "jc")
    names = matrix.nodes
    n = len(names)
    ctx.upload(synth200_packed, residues=False)
    top = Context.BETWEEN_MAX_GROUPS
    label = np.arange(n, dtype=np.int32) % top                             # = g: most groups are empty
    got = ctx.fill_affinity("jc", label, top, want_table=True)
    check(got, GroupAffinity.from_dense(matrix, [[names[g]] if g < n else [] for g in range(top)]), "G at the limit")
    assert (got["table"][0][:, n:] == 0).all() and (got["table"][1][:, n:] == EMPTY_ENTRY[1]).all() and (got["table"][2][:, n:] == -1).all()
    assert (got["near_group"] < n).all()
    high = np.zeros(n, dtype=np.int32)
    high[7], high[n - 1] = top - 1, top - 2                                # the table's last columns, reached from both directions
    got = ctx.fill_affinity("jc", high, top, want_table=True)
    check(got, GroupAffinity.from_dense(matrix, [[x for g, x in enumerate(names) if high[g] == a] for a in range(top)]), "the table's last columns")
    assert got["table"][1][0, top - 1] <= MILLION and got["table"][1][n - 2, top - 2] <= MILLION and got["table"][1][n - 1, top - 1] <= MILLION
    with pytest.raises(HipLibraryError, match=rf"status -4.*{top + 1}.*{top}"):
        ctx.fill_affinity("jc", label, top + 1)
    with pytest.raises(HipLibraryError, match="status -1.*genome 3 has label 5"):
        ctx.fill_affinity("jc", [0, 1, 2, 5] + [0] * (n - 4), 5)
    with pytest.raises(HipLibraryError, match="status -1.*genome 0 has label -1"):
        ctx.fill_affinity("jc", [-1] + [0] * (n - 1), 1)
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_affinity("jc", label, 0)
    with pytest.raises(HipLibraryError, match="status -1"):
        ctx.fill_affinity("jc", np.zeros(n, dtype=np.int32), 1, slab_bytes=-8)
    # by code, through the C-ABI: NULL group, a missing output pointer, peq before the residues; every output nulled
    from phamclust_amd.hip import _i32p, _i64p
    lib, h = ctx._lib, ctx._h
    zeros = np.zeros(n, dtype=np.int32)

    def call(metric, group=zeros, n_groups=1, with_lo=True, want_table=0):
        cells = [kind() for kind in (_i64p, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p, _i64p, _i32p, _i32p)]
        ns = ctypes.c_int32(7)
        refs = [ctypes.byref(cell) for cell in cells]
        if not with_lo:
            refs[1] = None
        rc = lib.pc_fill_affinity(h, metric, 1, group.ctypes.data_as(_i32p) if group is not None else None, n_groups, want_table, 0, *refs,
                                  ctypes.byref(ns), None)
        return rc, [bool(cell) for cell in cells], ns.value

    refused = ([False] * 10, 0)
    assert call(1, group=None) == (-1,) + refused
    assert call(1, with_lo=False) == (-1,) + refused
    assert call(5) == (-3,) + refused
    assert call(9) == (-1,) + refused
    assert call(1, n_groups=top + 1) == (-4,) + refused
    assert call(1) == (0, [True] * 7 + [False] * 3, 1)
    assert call(1, want_table=1) == (0, [True] * 10, 1)
    a, b, c = ctypes.c_float(-1.0), ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    assert lib.pc_last_affinity_times(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and a.value == b.value == c.value == 0.0      # no stats asked
    ctx.set_shard(1, 3)
    try:
        with pytest.raises(HipLibraryError, match="status -3"):
            ctx.fill_affinity("jc", zeros, 1)
    finally:
        ctx.set_shard(0, 1)
    # a loan ends with the next fill
    lent = ctx.fill_affinity("jc", zeros, 1, borrow=True)
    assert int(np.asarray(lent["own_sum"])[0]) == int(got["table"][0][0].sum())
    ctx.fill("jc")
    with pytest.raises(HipLibraryError):
        np.asarray(lent["own_sum"])
    # one genome: nothing runs on the device, every entry empty; no genome: nothing to upload at all
    ctx.upload(hand_built(1, "identical"))
    for g in (1, 3):
        got = ctx.fill_affinity("peq", [0], g, want_table=True, want_stats=True)
        assert got.pop("stats")["n_slabs"] == 0
        assert (got["own_sum"].tolist(), got["own_lo"].tolist(), got["own_hi"].tolist()) == tuple([v] for v in EMPTY_ENTRY)
        assert (got["near_sum"].tolist(), got["near_lo"].tolist(), got["near_hi"].tolist()) == tuple([v] for v in EMPTY_ENTRY)
        assert got["near_group"].tolist() == [[-1]] * 3 and [arr.tolist() for arr in got["table"]] == [[[v] * g] for v in EMPTY_ENTRY]
    with pytest.raises(ValueError):
        pack_genomes([])


# ---- 5: against an independent kernel ----------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "af", "peq"])
def test_folded_table_equals_the_between_fill(ctx, synth200_packed, metric):
    from phamclust_amd.matrix import GroupAffinity, GroupLinkage
    matrix = golden_matrix("synth200", metric)
    names = matrix.nodes
    ctx.upload(synth200_packed)
    for tag, groups in partitions(matrix).items():
        label = labels_of(names, groups)
        for as_distance in (True, False):
            got = ctx.fill_affinity(metric, label, len(groups), as_distance=as_distance, want_table=True, slab_bytes=8 * 4000)
            found = GroupAffinity(names, groups, *(got[name] for name in ARRAYS), table=got["table"], is_distance=as_distance)
            between = GroupLinkage(groups, *ctx.fill_between(metric, label, len(groups), as_distance=as_distance), is_distance=as_distance)
            assert found.folded() == between, (metric, tag, as_distance)


# ---- 6: several devices ------------------------------------------------------------------------------
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
            want = ctx.fill_affinity(metric, label, as_distance=as_distance, want_table=True)
            for slab_bytes in (0, 8 * 4000):
                got = multi.fill_affinity(metric, label, as_distance=as_distance, slab_bytes=slab_bytes, want_table=True, want_stats=True)
                st = got.pop("stats")
                same(got, want, (metric, world, tag, as_distance, slab_bytes))
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
            want = ctx.fill_affinity(metric, label, 3, want_table=True)
            got = multi.fill_affinity(metric, label, 3, slab_bytes=8, want_table=True, want_stats=True)
            st = got.pop("stats")
            same(got, want, (metric, label))
            assert st["stretches"][0] == 0 and st["stretches"][-1] == 3 and any(a == b for a, b in zip(st["stretches"], st["stretches"][1:]))
            assert st["n_pairs"] == 3
    multi.upload(hand_built(1, "chain"))
    got = multi.fill_affinity("jc", [0], 2, want_table=True)
    assert got["near_group"].tolist() == [[-1]] * 3 and (got["own_sum"].tolist(), got["own_lo"].tolist(), got["own_hi"].tolist()) == tuple([v] for v in EMPTY_ENTRY)
    assert [arr.tolist() for arr in got["table"]] == [[[v] * 2] for v in EMPTY_ENTRY]


# ---- 7: above the C-ABI ------------------------------------------------------------------------------
def test_affinity_de_novo(small_genomes, native_built):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    names = [g.name for g in small_genomes]
    dense = golden_matrix("small", "jc")
    assert dense.nodes == names
    groups = [names[r::4] for r in range(4)]
    found = M.affinity_de_novo(small_genomes, cli.METRICS["jc"], groups, want_table=True)
    assert found == M.GroupAffinity.from_dense(dense, groups) and M.LAST_FILL["metric"] == "jc" and M.LAST_FILL["n_slabs"] == 1
    by_index = M.affinity_de_novo(small_genomes, cli.METRICS["jc"], [list(range(r, len(names), 4)) for r in range(4)], as_distance=False, slab_bytes=8 * 40)
    assert by_index == M.GroupAffinity.from_dense(dense, groups, want_table=False).inverted() and M.LAST_FILL["n_slabs"] > 1
    assert by_index.medoids() == found.medoids()


def test_cluster_fit_run(tmp_path, small_genomes, native_built, monkeypatch):
    """--cluster-fit on the dense route and on --no-matrix: the two files, byte for byte the same on both routes and the host statement's
    over the final clusters; and everything else the run writes is what it writes without the flag."""
    from phamclust_amd.matrix import GroupAffinity
    from phamclust_amd.scripts.phamclust import main
    monkeypatch.setenv("PHAMCLUST_NO_HEATMAPS", "1")
    infile = os.path.join(GOLDEN, "small_input.tsv")
    new = ["cluster_fit_jc.tsv", "cluster_fit_jc_summary.tsv"]

    def run(tag, *flags):
        out = tmp_path / tag
        main([infile, str(out), "-m", "jc"] + list(flags))
        return out, {p.relative_to(out).as_posix(): p.read_bytes() for p in out.rglob("*") if p.is_file() and p.suffix != ".log"}

    plain_out, plain = run("plain")
    dense_out, dense = run("dense", "--cluster-fit")
    bare_out, bare = run("bare", "--no-matrix")
    sparse_out, sparse = run("sparse", "--no-matrix", "--cluster-fit")
    assert sorted(set(dense) - set(plain)) == new == sorted(set(sparse) - set(bare))
    assert {k: v for k, v in dense.items() if k not in new} == plain and {k: v for k, v in sparse.items() if k not in new} == bare
    for name in new:
        assert dense[name] == sparse[name] and len(dense[name]) > 0, name
    log_text = (dense_out / "phamclust.log").read_text()
    assert "cluster fit (affinity fill)" in log_text and "mean silhouette" in log_text
    # the files are the host statement's over the final clusters: cluster_1 .. cluster_k, then the singletons
    rows = [line.split("\t") for line in dense[new[0]].decode().splitlines()]
    assert rows[0] == ["genome", "cluster", "own_similarity", "nearest_cluster", "nearest_similarity", "silhouette", "medoid"]
    rows = rows[1:]
    assert sorted(row[0] for row in rows) == [g.name for g in small_genomes]
    order = []
    for row in rows:
        if row[1] not in order:
            order.append(row[1])
    groups = [[row[0] for row in rows if row[1] == cluster] for cluster in order]
    clusters = sorted((p.name for p in dense_out.iterdir() if p.is_dir() and p.name.startswith("cluster_")), key=lambda x: int(x.split("_")[1]))
    assert order[:len(clusters)] == clusters and all(len(group) == 1 and group[0] == cluster for group, cluster in zip(groups[len(clusters):], order[len(clusters):]))
    for cluster, group in zip(clusters, groups):
        assert sorted(group) == sorted(f.stem for f in (dense_out / cluster / "genomes").iterdir()), cluster
    want = GroupAffinity.from_dense(golden_matrix("small", "jc"), groups)
    similar = want.inverted()
    at = {x: k for k, x in enumerate(want.nodes)}
    silhouette, medoids = want.silhouette(), want.medoids()
    near, near_value = want.nearest_group("mean"), similar.nearest_value("mean")
    text = lambda v: "nan" if v != v else repr(float(v))                   # noqa: E731
    for row in rows:
        k, b = at[row[0]], order.index(row[1])
        assert row[2:] == [text(similar.own_mean(row[0])), order[near[k]] if near[k] >= 0 else "none", text(near_value[k]), text(silhouette[k]),
                           str(int(medoids[b] == row[0]))], row
    summary = [line.split("\t") for line in dense[new[1]].decode().splitlines()]
    assert summary[0] == ["cluster", "size", "medoid", "mean_silhouette", "largest_own_distance"] and len(summary) == 1 + len(groups)
    by_group = want.silhouette_by_group()
    for b, row in enumerate(summary[1:]):
        worst = max(int(want.own_hi[at[x]]) for x in groups[b])
        assert row == [order[b], str(len(groups[b])), medoids[b], text(by_group[b]), "nan" if worst < 0 else f"{worst / 1.0e6:.6f}"], row


def test_timing_tool_writes_its_lines(tmp_path, native_built):
    import subprocess
    import sys
    out = tmp_path / "affinity_fill.txt"
    tool = os.path.join(os.path.dirname(GOLDEN), "..", "tools", "affinity_timing.py")
    done = subprocess.run([sys.executable, tool, "--n", "300", "--n-peq", "120", "--repeats", "2", "--warmup", "1", "--out", str(out)],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    text = out.read_text()
    for workload in ("jc components", "peq components", "jc one group", "jc 2048 round-robin"):
        assert workload in text, text
    assert text.count("affinity: rows") == 4 and text.count("dense route: fill+D2H") == 4 and "ratio" in text
