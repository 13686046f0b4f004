"""The set-metric selector and its five kernel families at the sizes fills reach (MI355X): gcs / jc / pocp / af.

Every fill here is held to two things: its VALUES, `np.array_equal` against the oracle (`O.fill` whole matrices, `O.pairs` samples
plus a whole-matrix comparison with a second family where a whole oracle matrix would take too long) -- the oracle itself is pinned to
the live reference by tests/golden/ --, and its CHOICE: `Context.last_set_launch()` (the selector's inputs as the library gathered
them, the family, the launch shape) equals what tests/set_kernel_cases.py predicts from a numpy recount of the packed collection
through the library's host functions.  tests/test_host.py shows on the CPU that the cases below reach every coverage class a
default process can reach.
"""

import os

import numpy as np
import pytest

import set_kernel_cases as S

pytestmark = pytest.mark.gpu
KNOBS = ("PC_SET_KERNEL", "PC_POPC_TILE", "PC_S64_CHUNKS", "PC_COL_SEG")
N_SAMPLE = 200000


def _oracle():
    from oracle import oracle as O
    return O


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _set_knobs(**knobs):
    """Knobs the library reads per fill: PC_SET_KERNEL=..., PC_POPC_TILE=... (None / absent: unset)."""
    for name in KNOBS:
        os.environ.pop(name, None)
    for name, value in knobs.items():
        if value is not None:
            os.environ[name] = str(value)


def _assert_launch(ctx, stats, metric, owned=None):
    """The context's last set-metric fill ran what the cases module predicts for it: inputs, family and launch shape."""
    from phamclust_amd import hip
    forced = os.environ.get("PC_SET_KERNEL")
    fields, family, want = S.predict(hip.Context, stats, metric, owned, forced=forced, n_cu=_n_cu(), popc_tile=int(os.environ.get("PC_POPC_TILE", 0)),
                                     s64_chunks=int(os.environ.get("PC_S64_CHUNKS", 0)), col_seg=int(os.environ.get("PC_COL_SEG", 0)))
    inputs, shape = ctx.last_set_launch()
    assert ctx.last_set_kernel() == family == shape["family"], (metric, family, shape)
    assert shape == want, (metric, shape, want)
    assert {k: inputs[k] for k in fields} == fields and inputs["metric"] == metric and inputs["forced"] == forced, (inputs, fields)
    return family, shape


def _sample(n, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, N_SAMPLE), rng.integers(0, n, N_SAMPLE)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo < hi
    lo, hi = lo[keep], hi[keep]
    return lo, hi, lo * n - lo * (lo + 1) // 2 + (hi - lo - 1)


def _other_family(stats, metric, default):
    """A second family the guards admit for that fill."""
    from phamclust_amd import hip
    fields = S.selector_inputs(stats)
    for cand in ("sparse64", "popc", "sparsecol", "sparse", "walker"):
        if cand != default and hip.Context.set_kernel_choice(metric, forced=cand, **fields) == cand:
            return cand
    raise AssertionError((metric, default))


def _fill_dev(ctx, metric, dist, n_pairs):
    import torch
    out = torch.full((max(n_pairs, 1),), -1.0, dtype=torch.float64, device="cuda:0")
    ctx.fill_dev(metric, dist, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out[:n_pairs]


def _shard_columns(want, n, t_rank, t_lbase, rank, got):
    """Every column of the condensed matrix `want` that `rank` owns sits where the deal's table says in its shard `got`."""
    for t in range(1, n):
        if t_rank[t] == rank:
            s = np.arange(t)
            if not np.array_equal(got[t_lbase[t]:t_lbase[t] + t], want[s * n - s * (s + 1) // 2 + (t - s - 1)]):
                return t
    return None


# shards of these run another family than the whole matrix does (area = N x owned targets): what `phamclust --gpus N` meets
SHARDS_CHANGE_FAMILY = ("real3000", "uniform2300", "col4100", "many8192")


@pytest.mark.parametrize("name", list(S.CASES))
def test_default_choice_whole_and_sharded(gpu_ctx, native_built, name):
    """No PC_SET_KERNEL: the selector's own choice on a designed collection, distance and similarity, equals the oracle and runs the
    family and launch shape predicted for it; then every rank of its worlds under the boustrophedon and the cost-balanced deal fills
    its shard (family and shape predicted per rank from ITS owned targets), and the assembled shards equal the unsharded matrix;
    last, one MultiContext([0, 0, 0]) fill for jc and af gives that matrix too."""
    import torch
    from phamclust_amd import hip
    O = _oracle()
    metrics, worlds, mode = S.CASES[name]
    packed, stats = S.collection(name)
    n, n_pairs = packed.n_genomes, packed.n_pairs
    stream = torch.cuda.current_stream().cuda_stream
    _set_knobs()
    try:
        gpu_ctx.upload(packed, residues=False)
        gpu_ctx.set_shard(0, 1)
        whole, whole_family = {}, {}
        lo, hi, idx = _sample(n, 7 + n)
        idx_dev = torch.from_numpy(idx).to("cuda:0")
        for metric in metrics:
            for dist in (True, False):
                got = _fill_dev(gpu_ctx, metric, dist, n_pairs)
                family, _ = _assert_launch(gpu_ctx, stats, metric)
                assert family == S.EXPECTED_WHOLE[name][S.SET_METRICS.index(metric)], (name, metric, family)
                if mode == "whole":
                    assert np.array_equal(got.cpu().numpy(), O.fill(packed, metric, dist)), (name, metric, dist, family)
                else:
                    assert np.array_equal(got[idx_dev].cpu().numpy(), O.pairs(packed, metric, lo, hi, as_distance=dist)), (name, metric, dist, family)
                    other = _other_family(stats, metric, family)
                    _set_knobs(PC_SET_KERNEL=other)
                    again = _fill_dev(gpu_ctx, metric, dist, n_pairs)
                    assert _assert_launch(gpu_ctx, stats, metric)[0] == other != family
                    _set_knobs()
                    assert torch.equal(got, again), (name, metric, dist, family, other)
                    del again
                if dist:
                    whole[metric], whole_family[metric] = got, family
        changed = set()
        costs = S.target_costs(packed) if worlds else None
        for world in worlds:
            for balanced in S.DEALS:
                owned = [S.owned_targets(packed, r, world, balanced, costs) for r in range(world)]
                for metric in metrics:
                    gathered, stride = None, None
                    for rank in range(world):
                        gpu_ctx.set_shard(rank, world, balanced=balanced)
                        if gathered is None:
                            stride = gpu_ctx.shard_stride()
                            gathered = torch.full((world * stride,), -1.0, dtype=torch.float64, device="cuda:0")
                            t_rank, _ = gpu_ctx.shard_table()
                            assert all(np.array_equal(np.flatnonzero(t_rank == r), owned[r]) for r in range(world)), (name, world, balanced)
                        assert gpu_ctx.shard_stride() == stride
                        gpu_ctx.fill_shard_dev(metric, True, gathered[rank * stride:].data_ptr(), stream, want_stats=False)
                        torch.cuda.synchronize()
                        family, _ = _assert_launch(gpu_ctx, stats, metric, owned[rank])
                        if family != whole_family[metric]:
                            changed.add((metric, world, family))
                    out = torch.full((n_pairs,), -2.0, dtype=torch.float64, device="cuda:0")
                    gpu_ctx.assemble_dev(gathered.data_ptr(), world, out.data_ptr(), stream)
                    torch.cuda.synchronize()
                    assert torch.equal(out, whole[metric]), (name, metric, world, balanced)
                    del gathered, out
        gpu_ctx.set_shard(0, 1)
        if name in SHARDS_CHANGE_FAMILY:
            assert changed, name
        if worlds == S.WORLDS:
            with hip.MultiContext([0, 0, 0]) as multi:
                multi.upload(packed, residues=False)
                for metric in ("jc", "af"):
                    if metric in metrics:
                        assert np.array_equal(np.asarray(multi.fill(metric)), whole[metric].cpu().numpy()), (name, metric)
    finally:
        _set_knobs()
        gpu_ctx.set_shard(0, 1)
        S.forget(name)


FORCED = (("popc", 32), ("popc", 64), ("sparse", None), ("sparse64", None), ("walker", None))


@pytest.mark.parametrize("n_genomes", [31, 32, 33, 63, 64, 65, 127, 129])
def test_every_family_forced_at_tile_edges(gpu_ctx, native_built, n_genomes):
    """Both popcount tiles, the 32 x 32 and 64 x 64 sparse tiles and the walker, forced, at one genome fewer than a tile, exactly a
    tile and one more (32 and 64), and two tiles of 64 but one: all four metrics where the family exists for them, both polarities,
    unsharded and as the two shards of a 2-rank deal; every value against the oracle.  (The column kernel:
    test_column_kernel_edge_sizes.)"""
    import torch
    from phamclust_amd.synth import synth_packed
    O = _oracle()
    packed = synth_packed(n_genomes, 700, seed=300 + n_genomes)
    stats = S.recount(packed)
    want = {(m, d): O.fill(packed, m, d) for m in S.SET_METRICS for d in (True, False)}
    stream = torch.cuda.current_stream().cuda_stream
    try:
        gpu_ctx.upload(packed, residues=False)
        for family, tile in FORCED:
            _set_knobs(PC_SET_KERNEL=family, PC_POPC_TILE=tile)
            metrics = [m for m in S.SET_METRICS if not (family == "popc" and m == "af") and not (family in ("sparse", "walker") and m in ("gcs", "jc"))]
            gpu_ctx.set_shard(0, 1)
            for m in metrics:
                for dist in (True, False):
                    assert np.array_equal(gpu_ctx.fill(m, dist), want[(m, dist)]), (family, tile, m, dist)
                    ran, shape = _assert_launch(gpu_ctx, stats, m)
                    assert ran == family and (tile is None or shape["tile"] == tile)
            for balanced in S.DEALS:
                for rank in range(2):
                    gpu_ctx.set_shard(rank, 2, balanced=balanced)
                    t_rank, t_lbase = gpu_ctx.shard_table()
                    owned = np.flatnonzero(t_rank == rank)
                    for m in metrics:
                        buf = torch.full((max(gpu_ctx.shard_stride(), 1),), -1.0, dtype=torch.float64, device="cuda:0")
                        gpu_ctx.fill_shard_dev(m, True, buf.data_ptr(), stream, want_stats=False)
                        torch.cuda.synchronize()
                        assert _assert_launch(gpu_ctx, stats, m, owned)[0] == family
                        assert _shard_columns(want[(m, True)], n_genomes, t_rank, t_lbase, rank, buf.cpu().numpy()) is None, (family, tile, m, rank, balanced)
    finally:
        _set_knobs()
        gpu_ctx.set_shard(0, 1)


def _edge_want(subset):
    """{(metric, as_distance): the live reference's values} for a sub-collection of the numeric-edge genomes."""
    from test_host import set_edges_fixture
    full = set_edges_fixture()
    return {key: S.sub_condensed(vec, list(S.EDGE_NAMES), S.EDGE_SUBSETS[subset]) for key, vec in full.items()}


# what the guards admit, stated by hand: subset -> {metric: families that must run when forced}; every other forced family must
# be refused (the fill runs the default choice instead)
EDGE_ADMITTED = {
    "lo": {"gcs": {"popc", "sparse64", "sparsecol"}, "jc": {"popc", "sparse64", "sparsecol"},
           "pocp": {"popc", "sparse", "sparse64", "walker", "sparsecol"}, "af": {"sparse", "sparse64", "walker", "sparsecol"}},
    # 65,536 genes: pocp's 16-bit packings are out; an entry of 65,536 residues: af's column kernel is out
    "hi": {"gcs": {"popc", "sparse64", "sparsecol"}, "jc": {"popc", "sparse64", "sparsecol"},
           "pocp": {"popc", "sparse", "walker"}, "af": {"sparse", "sparse64", "walker"}},
    # an empty translation: af's "sum == 0" kernels are out
    "empty": {"gcs": {"popc", "sparse64", "sparsecol"}, "jc": {"popc", "sparse64", "sparsecol"},
              "pocp": {"popc", "sparse", "sparse64", "walker", "sparsecol"}, "af": {"sparse", "walker"}},
    "all": {"gcs": {"popc", "sparse64", "sparsecol"}, "jc": {"popc", "sparse64", "sparsecol"},
            "pocp": {"popc", "sparse", "walker"}, "af": {"sparse", "walker"}},
}
EDGE_DEFAULT = {"lo": {"gcs": "popc", "jc": "popc", "pocp": "popc", "af": "sparse64"}, "hi": {"gcs": "popc", "jc": "popc", "pocp": "popc", "af": "sparse64"},
                "empty": {"gcs": "popc", "jc": "popc", "pocp": "popc", "af": "sparse"}, "all": {"gcs": "popc", "jc": "popc", "pocp": "popc", "af": "sparse"}}


@pytest.mark.parametrize("subset", ["lo", "hi", "empty", "all"])
def test_numeric_edges_every_admitted_family(gpu_ctx, native_built, subset):
    """Genomes on the selector's numeric guards (65,535 / 65,536 genes, entries of 65,535 / 65,536 residues, an empty translation;
    1,447 / 1,448 phams ride along): the default choice, then every family forced -- the ones the guards admit must run, the others
    must be refused -- and both popcount tiles; every value equals what the LIVE reference wrote (tests/golden/set_edges/)."""
    want = _edge_want(subset)
    packed = S.edge_packed(subset)
    stats = S.recount(packed)
    try:
        gpu_ctx.upload(packed, residues=False)
        gpu_ctx.set_shard(0, 1)
        for forced in (None,) + S.FAMILIES:
            for tile in ((32, 64) if forced == "popc" else (None,)):
                _set_knobs(PC_SET_KERNEL=forced, PC_POPC_TILE=tile)
                for m in S.SET_METRICS:
                    for dist in (True, False):
                        got = gpu_ctx.fill(m, dist)
                        assert np.array_equal(got, want[(m, dist)]), (subset, forced, tile, m, dist, gpu_ctx.last_set_kernel())
                        ran, _ = _assert_launch(gpu_ctx, stats, m)
                        if forced is None or forced not in EDGE_ADMITTED[subset][m]:
                            assert ran == EDGE_DEFAULT[subset][m], (subset, forced, m, ran)
                        else:
                            assert ran == forced, (subset, forced, m, ran)
    finally:
        _set_knobs()


def test_epilogue_table_and_its_reuse_key(gpu_ctx, native_built):
    """The popcount tiles' epilogue table on both sides of its 4 Mi entries -- 1,447 / 1,448 phams for gcs / jc, 1,023 / 1,024 genes
    for pocp -- on both tiles, and its reuse: the table is rebuilt when metric, polarity or the collection's maximum changes and only
    then, so fills that alternate all three on ONE context must each give the reference's values."""
    want = {name: _edge_want(name) for name in ("phams1447", "phams1448", "genes1023", "genes1024")}
    packs = {name: S.edge_packed(name) for name in want}
    stats = {name: S.recount(p) for name, p in packs.items()}
    expect_table = {("phams1447", "gcs"): 1, ("phams1447", "jc"): 1, ("phams1448", "gcs"): 0, ("phams1448", "jc"): 0,
                    ("genes1023", "pocp"): 1, ("genes1024", "pocp"): 0, ("genes1023", "jc"): 1, ("genes1024", "gcs"): 1,
                    ("phams1447", "pocp"): 0, ("phams1448", "pocp"): 0}
    seen = set()
    try:
        for tile in (32, 64):
            _set_knobs(PC_SET_KERNEL="popc", PC_POPC_TILE=tile)
            # two passes over uploads with different maxima; inside, metric and polarity alternate so that consecutive fills differ in one key part
            for name in ("phams1447", "genes1023", "phams1448", "genes1024", "phams1447", "genes1024", "genes1023"):
                gpu_ctx.upload(packs[name], residues=False)
                for m, dist in (("jc", True), ("jc", False), ("gcs", False), ("pocp", False), ("pocp", True), ("gcs", True), ("jc", True), ("pocp", True)):
                    got = gpu_ctx.fill(m, dist)
                    ran, shape = _assert_launch(gpu_ctx, stats[name], m)
                    assert ran == "popc" and shape["tile"] == tile
                    if (name, m) in expect_table:
                        assert shape["table"] == expect_table[(name, m)], (name, m, shape)
                    seen.add((S.metric_group(m), shape["table"], tile))
                    assert np.array_equal(got, want[name][(m, dist)]), (tile, name, m, dist)
        assert seen == {(g, t, tile) for g in ("counts", "pocp") for t in (0, 1) for tile in (32, 64)}
    finally:
        _set_knobs()


def _holder_pairs(n_genomes, n_phams, seed, per_extra=0):
    """`n_phams` phams, each held by exactly two genomes (pham p: genome p mod N and a second one that moves with p / N), one to four
    genes each with translations of 1 ... 39 residues, plus a pham of its own per genome: the two-holder count is n_phams exactly."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    rng = np.random.default_rng(seed)
    held = [[] for _ in range(n_genomes)]
    for p in range(n_phams):
        a = p % n_genomes
        b = (a + 1 + (p // n_genomes) % (n_genomes - 1)) % n_genomes
        held[a].append(p)
        held[b].append(p)
    genomes = []
    for k in range(n_genomes):
        g = Genome(f"g{k:04d}")
        for p in held[k]:
            for _ in range(int(rng.integers(2, 5)) if p % 7 == 0 else 1):
                g.add(f"p{p:05d}", "M" * int(rng.integers(1, 40)))
        g.add(f"own{k:04d}", "MK")
        genomes.append(g)
    return pack_genomes(genomes)


@pytest.mark.parametrize("family,metrics,limit,n_genomes", [("sparsecol", ("gcs", "jc"), 7872, 200), ("sparsecol", ("pocp", "af"), 6272, 784),
                                                           ("sparse64", ("af",), 6912, 200), ("sparse64", ("gcs", "jc", "pocp"), 7680, 200)])
def test_mask_capacity_and_one_past(gpu_ctx, native_built, family, metrics, limit, n_genomes):
    """Phams with two holders at a kernel's mask capacity and one past it: the column kernel takes 7,872 (gcs / jc) and 6,272
    (pocp / af: with 784 genomes a block's 1,024 entries fit the 1,151 its value table then holds) and must be refused one pham
    later; the 64 x 64 sparse tiles hold 7,680 in one chunk (af's broadcast-staging instance 6,912) and split one pham later."""
    O = _oracle()
    try:
        for count in (limit, limit + 1):
            packed = _holder_pairs(n_genomes, count, seed=count)
            stats = S.recount(packed)
            assert stats["two_holder"] == count
            gpu_ctx.upload(packed, residues=False)
            gpu_ctx.set_shard(0, 1)
            for m in metrics:
                for dist in (True, False):
                    _set_knobs(PC_SET_KERNEL=family)
                    got = gpu_ctx.fill(m, dist)
                    ran, shape = _assert_launch(gpu_ctx, stats, m)
                    if family == "sparsecol":
                        assert (ran == "sparsecol") == (count == limit), (m, count, ran)
                        if count == limit and m in ("pocp", "af"):
                            assert shape["vals_cap"] == 1151 and stats["max_ent_len"] < 65536 and S.block_entries(stats).max() <= 1151
                    else:
                        assert ran == "sparse64" and shape["chunks"] == (1 if count == limit else 2), (m, count, shape)
                        assert shape["batches"] == (2 if count == limit else 1) and shape["dense"] == (1 if m == "af" and count == limit else 0)
                    assert np.array_equal(got, O.fill(packed, m, dist)), (family, m, dist, count, ran)
    finally:
        _set_knobs()


def _value_table_case(light):
    """128 genomes, 5,056 phams with two holders (value-table cap 7,231): genome g < 64 holds 113 consecutive phams from 79 g
    (the genomes in `light` 112) and genome g + 64 the same ones, so both unsharded blocks hold 64 x 113 - (light genomes below
    64) entries."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    rng = np.random.default_rng(128)
    genomes = []
    for k in range(128):
        g = Genome(f"g{k:04d}")
        for j in range(112 if k in light else 113):
            p = ((k % 64) * 79 + j) % 5056
            for _ in range(3 if p % 9 == 0 else 1):
                g.add(f"p{p:05d}", "M" * int(rng.integers(1, 40)))
        genomes.append(g)
    return pack_genomes(genomes)


def test_value_table_cap_exactly_and_one_past(gpu_ctx, native_built):
    """A block of 64 targets holding exactly the 7,231 entries the column kernel's LDS value table takes at 5,056 mask entries, and
    7,232: pocp / af run the column kernel in the first case and must leave it in the second, gcs / jc never care.  As a 2-rank
    shard the blocks are other genomes than the unsharded ones: of the exact collection, rank 1 (which owns both light genomes)
    keeps 7,230 and stays, rank 0 holds 7,232 and leaves -- the selector counts the rank's OWN blocks."""
    import torch
    O = _oracle()
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for light, blocks in (((5, 69), 7231), ((69,), 7232)):
            packed = _value_table_case(light)
            stats = S.recount(packed)
            assert stats["two_holder"] == 5056 and int(S.block_entries(stats).max()) == blocks
            gpu_ctx.upload(packed, residues=False)
            _set_knobs(PC_SET_KERNEL="sparsecol")
            gpu_ctx.set_shard(0, 1)
            want = {(m, d): O.fill(packed, m, d) for m in S.SET_METRICS for d in (True, False)}
            for (m, dist), w in want.items():
                got = gpu_ctx.fill(m, dist)
                ran, shape = _assert_launch(gpu_ctx, stats, m)
                assert (ran == "sparsecol") == (m in ("gcs", "jc") or blocks == 7231), (m, blocks, ran)
                assert ran != "sparsecol" or m in ("gcs", "jc") or shape["vals_cap"] == 7231
                assert np.array_equal(got, w), (m, dist, blocks, ran)
            if blocks != 7231:
                continue
            for rank in range(2):
                gpu_ctx.set_shard(rank, 2)
                t_rank, t_lbase = gpu_ctx.shard_table()
                owned = np.flatnonzero(t_rank == rank)
                own_blocks = int(S.block_entries(stats, owned).max())
                assert own_blocks == (7232 if rank == 0 else 7230)
                for m in S.SET_METRICS:
                    buf = torch.full((gpu_ctx.shard_stride(),), -1.0, dtype=torch.float64, device="cuda:0")
                    gpu_ctx.fill_shard_dev(m, True, buf.data_ptr(), stream, want_stats=False)
                    torch.cuda.synchronize()
                    ran, _ = _assert_launch(gpu_ctx, stats, m, owned)
                    assert (ran == "sparsecol") == (m in ("gcs", "jc") or rank == 1), (m, rank, ran)
                    assert _shard_columns(want[(m, True)], 128, t_rank, t_lbase, rank, buf.cpu().numpy()) is None, (m, rank)
    finally:
        _set_knobs()
        gpu_ctx.set_shard(0, 1)


def test_column_kernel_forced_seg_1_and_64(gpu_ctx, native_built):
    """PC_COL_SEG = 1 and 64 on synth(4100, 5000): 65 source tiles, so one run per tile and two runs (64 tiles + 1) -- both must
    give the matrix of the default launch (2 tiles per unit), which test_default_choice_whole_and_sharded[col4100] holds to the
    oracle whole; here 200,000 pairs are."""
    import torch
    O = _oracle()
    packed, stats = S.collection("col4100")
    n = packed.n_genomes
    lo, hi, idx = _sample(n, 41)
    idx_dev = torch.from_numpy(idx).to("cuda:0")
    try:
        gpu_ctx.upload(packed, residues=False)
        gpu_ctx.set_shard(0, 1)
        for m in S.SET_METRICS:
            _set_knobs()
            base = _fill_dev(gpu_ctx, m, True, packed.n_pairs)
            assert _assert_launch(gpu_ctx, stats, m)[1]["seg"] == 2
            assert np.array_equal(base[idx_dev].cpu().numpy(), O.pairs(packed, m, lo, hi, as_distance=True)), m
            for seg, runs in ((1, 65), (64, 2)):
                _set_knobs(PC_COL_SEG=seg)
                got = _fill_dev(gpu_ctx, m, True, packed.n_pairs)
                ran, shape = _assert_launch(gpu_ctx, stats, m)
                assert ran == "sparsecol" and (shape["seg"], shape["runs"]) == (seg, runs)
                assert torch.equal(got, base), (m, seg)
    finally:
        _set_knobs()
        S.forget("col4100")
