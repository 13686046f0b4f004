"""The rows forms of the edge-list, components and tree fills (pc_fill_rows_edges / _components / _tree, Context.fill_rows_*,
edges_extend / components_extend / tree_extend, --grow) on the GPU (run with ``-m gpu``).

A stored result over a subset of the genomes is grown by the others.  The stored result and the expected one both come from a DENSE
vector -- a golden file the live reference wrote, or the same context's whole fill, which the rest of the suite pins -- through the
``from_dense`` host statements, as tests/test_gpu_tree.py does; tests/test_rows_slabs_host.py holds the ``extended`` statements to
them.  Every assertion is exact: ``np.array_equal`` on indices and on the bits of values.  A pair of two new genomes taken twice or
not at all, a diagonal taken for a pair, a (row, column) carried wrongly over a row end or a workgroup seam, a seed forest that is
dropped or re-indexed wrongly, an orientation that follows the row instead of the order, or a tie resolved by the row order fails here."""

import os

import numpy as np
import pytest

from conftest import ALL_METRICS, golden_file, read_lower_triangle, synth200_file

pytestmark = pytest.mark.gpu

PASSES = ("edges", "components", "tree")


@pytest.fixture()
def ctx(gpu_ctx):
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    yield gpu_ctx
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def square_of(condensed, n, as_distance):
    full = np.zeros((n, n))
    full[np.triu_indices(n, k=1)] = np.asarray(condensed)
    full = full + full.T
    np.fill_diagonal(full, 0.0 if as_distance else 1.0)
    return full


class Dense:
    """A dense matrix over n genomes and what the host statements say of it and of its blocks (computed once per key)."""

    def __init__(self, square, as_distance):
        self.square, self.as_distance, self.n = square, as_distance, square.shape[0]
        self.names = [f"n{k:05d}" for k in range(self.n)]
        self._memo = {}

    def matrix(self, at):
        from phamclust_amd.matrix import _square_matrix
        at = np.asarray(at, dtype=np.int64)
        return _square_matrix([self.names[g] for g in at.tolist()], self.square[np.ix_(at, at)].copy(), self.as_distance)

    def get(self, kind, at, *args):
        from phamclust_amd.matrix import SingleLinkageTree, SparseEdges
        key = (kind, tuple(at), args)
        if key not in self._memo:
            if kind == "tree":
                self._memo[key] = SingleLinkageTree.from_dense(self.matrix(at))
            elif kind == "edges":
                self._memo[key] = SparseEdges.from_dense(self.matrix(at), args[0])
            else:
                wide = 2.0 if self.as_distance else -1.0
                self._memo[key] = SparseEdges.from_dense(self.matrix(at), wide).components(args[0], args[1])
        return self._memo[key]

    def passing_new_pairs(self, new, threshold, strict=False):
        """Pairs that touch a genome of ``new`` and pass, each once."""
        s, t = np.triu_indices(self.n, k=1)
        is_new = np.zeros(self.n, dtype=bool)
        is_new[new] = True
        w = self.square[s, t]
        if self.as_distance:
            ok = w < threshold if strict else w <= threshold
        else:
            ok = w > threshold if strict else w >= threshold
        return int((ok & (is_new[s] | is_new[t])).sum())


def grow_all(ctx, metric, dense, new, threshold, slab_bytes=0, label=None, want_slabs=None):
    """The three rows forms from the stored results of the old block, each held to the host statement of the whole matrix."""
    n, as_distance = dense.n, dense.as_distance
    new = sorted(int(g) for g in new)
    old = np.asarray([g for g in range(n) if g not in set(new)], dtype=np.int64)
    everyone = list(range(n))
    label = (label, metric, as_distance, tuple(new) if len(new) < 8 else len(new), threshold, slab_bytes)
    # tree
    stored, want = dense.get("tree", old), dense.get("tree", everyone)
    seed = (old[stored.source], old[stored.target], stored.weight)
    src, tgt, val, st = ctx.fill_rows_tree(metric, new, seed=seed, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
    assert src.dtype == np.int32 and tgt.dtype == np.int32 and val.dtype == np.float64, label
    assert np.array_equal(src, want.source) and np.array_equal(tgt, want.target) and same_bits(val, want.weight), label
    assert st["n_edges"] == n - 1, label
    if want_slabs is not None:
        assert st["n_slabs"] == want_slabs, label
    # components, both predicates
    for strict in (True, False):
        stored, want = dense.get("components", old, threshold, strict), dense.get("components", everyone, threshold, strict)
        seed_labels = np.arange(n, dtype=np.int32)
        seed_labels[old] = old[stored]
        labels, st = ctx.fill_rows_components(metric, threshold, new, seed_labels=seed_labels, as_distance=as_distance, strict=strict,
                                              slab_bytes=slab_bytes, want_stats=True)
        assert labels.dtype == np.int32 and np.array_equal(labels, want), label + (strict,)
        assert st["n_edges"] == dense.passing_new_pairs(new, threshold, strict), label + (strict,)
        assert st["n_components"] == len(set(want.tolist())), label + (strict,)
        if want_slabs is not None:
            assert st["n_slabs"] == want_slabs, label
    # edges: the call's list alone, then merged with the stored one
    stored, want = dense.get("edges", old, threshold), dense.get("edges", everyone, threshold)
    src, tgt, val, st = ctx.fill_rows_edges(metric, threshold, new, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
    assert st["n_edges"] == src.shape[0] == dense.passing_new_pairs(new, threshold), label     # a pair taken twice or dropped fails here
    assert (src < tgt).all() and np.array_equal(np.lexsort((src, tgt)), np.arange(src.shape[0])), label
    s = np.concatenate([old[stored.source], src])
    t = np.concatenate([old[stored.target], tgt])
    w = np.concatenate([stored.weight, val])
    order = np.lexsort((s, t))
    assert np.array_equal(s[order], want.source) and np.array_equal(t[order], want.target) and same_bits(w[order], want.weight), label
    if want_slabs is not None:
        assert st["n_slabs"] == want_slabs, label


def old_subsets(n):
    """The new genomes of: all but first, all but last, all but two adjacent middle ones, only one old genome, every second genome old."""
    return {"first": [0], "last": [n - 1], "middle": [n // 2, n // 2 + 1], "one_old": [g for g in range(n) if g != 5], "second": list(range(1, n, 2))}


_GOLDEN = {}


def golden_dense(ctx, metric, as_distance):
    key = (metric, as_distance)
    if key not in _GOLDEN:
        if as_distance:
            _, values, _ = read_lower_triangle(golden_file(metric))
        else:
            values = ctx.fill(metric, as_distance=False)
        _GOLDEN[key] = Dense(square_of(values, ctx.n_genomes, as_distance), as_distance)
    return _GOLDEN[key]


# ---- 1: all six metrics on the 23 golden genomes ------------------------------------------------------------------
@pytest.mark.parametrize("metric", ALL_METRICS)
def test_golden_collection_grown_from_every_subset(ctx, small_packed, metric):
    """aai is not symmetric: a pair oriented by its row instead of by the order fails.  jc and peq also as similarities."""
    ctx.upload(small_packed)
    n = small_packed.n_genomes
    for as_distance in ((True, False) if metric in ("jc", "peq") else (True,)):
        dense = golden_dense(ctx, metric, as_distance)
        for name, new in old_subsets(n).items():
            grow_all(ctx, metric, dense, new, 0.75 if as_distance else 0.25, label=name)


def test_the_golden_inputs_are_not_vacuous(ctx, small_packed):
    """Asserted from the dense expectation.  jc distances of the 23 golden genomes, the two adjacent middle genomes (11, 12) new:
    at d < 0.55 the old 21 genomes fall into 9 components and the 23 into 7 -- new genomes join old components (at d < 0.75 none
    does: 3 and 3) -- and the grown tree keeps 14 of the stored tree's 20 edges: new pairs replace six."""
    ctx.upload(small_packed)
    n = small_packed.n_genomes
    dense = golden_dense(ctx, "jc", True)
    new = old_subsets(n)["middle"]
    old = np.asarray([g for g in range(n) if g not in new])
    stored, grown = dense.get("components", old, 0.55, True), dense.get("components", list(range(n)), 0.55, True)
    bridged = [c for c in set(grown.tolist()) if len({int(stored[k]) for k, g in enumerate(old.tolist()) if grown[g] == c}) >= 2]
    assert bridged, "no new genome joins two old components at this threshold"
    stored, grown = dense.get("tree", old), dense.get("tree", list(range(n)))
    seed = set(zip(old[stored.source].tolist(), old[stored.target].tolist()))
    kept = sum((s, t) in seed for s, t in zip(grown.source.tolist(), grown.target.tolist()))
    assert kept < len(seed) == n - 3, "no new pair replaces an edge of the stored tree"
    grow_all(ctx, "jc", dense, new, 0.55, label="bridging")


# ---- 2: synth200, the slab cut ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["jc", "pocp", "peq"])
def test_synth200_under_every_slab_cut(ctx, synth200_packed, metric):
    from phamclust_amd.hip import Context
    ctx.upload(synth200_packed)
    n = synth200_packed.n_genomes
    _, values, _ = read_lower_triangle(synth200_file(metric))
    dense = Dense(square_of(values, n, True), True)
    new = [3, 4, 60, 97, 131, 198, 199]
    for slab_bytes, want in ((8 * n, 7), (8 * n * 2, 4), (8 * n * 3, 3), (0, 1)):
        if slab_bytes:
            assert Context.rows_slabs(n, len(new), slab_bytes) == want
        grow_all(ctx, metric, dense, new, 0.9, slab_bytes=slab_bytes, want_slabs=want, label="synth200")


# ---- 3: workgroup seams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_workgroup_seams(ctx, n):
    """m rows of n values against one workgroup's span of each pass: the largest m with m * n <= span and the first above it (n = 65:
    4,095 and 4,160 values; n = 64: 4,032, 4,096 and all 64 rows; n = 129: 3,999 / 4,128 and, two spans, 8,127 / 8,256), whole and
    cut into two slabs, so that pairs of two new genomes lie in different slabs and must be taken once.  n = 65 runs its counts a second
    time on the similarity form (sim >= 0.1, expected from the similarity fill)."""
    from phamclust_amd.hip import Context
    from phamclust_amd.synth import synth_packed
    spans = {Context.rows_pass_span(kind) for kind in PASSES}
    ctx.upload(synth_packed(n, 300, seed=n), residues=False)
    dense = Dense(square_of(ctx.fill("jc"), n, True), True)
    counts = set()
    for span in spans:
        assert span > 0
        for k in (1, 2):
            m = k * span // n
            counts.update(min(x, n) for x in (m - 1 if (k * span) % n == 0 else None, m, m + 1) if x is not None)      # (n = 63: all 63 rows, 3,969 values)
    assert counts and min(counts) >= 1
    forms = [(dense, 0.9)]
    if n == 65:     # once more as similarities: the passes' similarity instances meet a workgroup seam of a rows slab only here
        forms.append((Dense(square_of(ctx.fill("jc", as_distance=False), n, False), False), 0.1))
    for dense, thr in forms:
        sim = {} if dense.as_distance else {"as_distance": False}
        for m in sorted(counts):
            new = sorted(np.random.default_rng(m).choice(n, size=m, replace=False).tolist()) if m < n else list(range(n))
            if m == n:                                                      # every genome new: nothing stored
                src, tgt, val = ctx.fill_rows_tree("jc", new, **sim)
                want = dense.get("tree", list(range(n)))
                assert np.array_equal(src, want.source) and np.array_equal(tgt, want.target) and same_bits(val, want.weight)
                s, t, v, st = ctx.fill_rows_edges("jc", thr, new, want_stats=True, **sim)
                want = dense.get("edges", list(range(n)), thr)
                assert np.array_equal(s, want.source) and np.array_equal(t, want.target) and same_bits(v, want.weight) and st["n_slabs"] == 1
                labels = ctx.fill_rows_components("jc", thr, new, **sim)
                assert np.array_equal(labels, dense.get("components", list(range(n)), thr, True))
                continue
            grow_all(ctx, "jc", dense, new, thr, label=("seam", n, m), want_slabs=1)
            half = (m + 1) // 2
            grow_all(ctx, "jc", dense, new, thr, slab_bytes=8 * n * half, label=("seam, two slabs", n, m), want_slabs=2 if m > 1 else 1)


# ---- 4: ties and contention ---------------------------------------------------------------------------------------
def hand_built(n, twins=()):
    """n genomes of a chain -- genome k holds phams p{k} and p{k+1}, so only neighbours share one, all the same way -- or, with
    ``twins`` = "all", n identical genomes; else one more genome per entry of ``twins``, identical to that genome of the chain."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        if twins == "all":
            for j in range(4):
                g.add(f"p{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        else:
            g.add(f"p{k}", "MKTAYIAKQRQISFVKSHFSRQ")
            g.add(f"p{k + 1}", "MKTAYLAKQRQISWVKSHFARQ")
        genomes.append(g)
    if twins != "all":
        for i, k in enumerate(twins):
            g = Genome(f"g{n + i:04d}")
            g.add(f"p{k}", "MKTAYIAKQRQISFVKSHFSRQ")
            g.add(f"p{k + 1}", "MKTAYLAKQRQISWVKSHFARQ")
            genomes.append(g)
    return pack_genomes(genomes)


def test_identical_genomes_every_key_ties(ctx):
    """65 identical genomes and 3 new ones: every key ties on its value and every hook lands on genome 0; the tree is the star at 0."""
    n = 68
    ctx.upload(hand_built(n, "all"))
    for metric in ("jc", "peq"):
        dense = Dense(square_of(ctx.fill(metric), n, True), True)
        assert (dense.square == 0.0).all()
        want = dense.get("tree", list(range(n)))
        assert want.source.tolist() == [0] * (n - 1) and want.target.tolist() == list(range(1, n))
        for new in ([0, 30, 67], [1, 2, 3]):
            grow_all(ctx, metric, dense, new, 0.5, label="identical")
            grow_all(ctx, metric, dense, new, 0.5, slab_bytes=8 * n, label="identical, a row per slab", want_slabs=3)


def test_a_new_genome_identical_to_an_old_one(ctx):
    """A chain of 40 and two more genomes, twins of genomes 7 and 21 of the chain: each twin ties with its original on every value, so
    the tree's tie order (the smaller target, then the smaller source) decides which of them an edge names."""
    n = 42
    ctx.upload(hand_built(40, twins=(7, 21)))
    for metric in ("jc", "peq"):
        dense = Dense(square_of(ctx.fill(metric), n, True), True)
        assert dense.square[7, 40] == 0.0 and dense.square[21, 41] == 0.0 and np.array_equal(dense.square[7, :7], dense.square[40, :7])
        for new in ([40, 41], [7, 41], [7, 21], [6, 7, 8, 40]):
            grow_all(ctx, metric, dense, new, 0.95, label="twins")
            grow_all(ctx, metric, dense, new, 0.95, slab_bytes=8 * n, label="twins, a row per slab", want_slabs=len(new))


# ---- 5: the seed's domain, no query row ---------------------------------------------------------------------------
def test_seed_domain_and_no_rows(ctx, small_packed):
    from phamclust_amd.hip import HipLibraryError
    ctx.upload(small_packed)
    n = small_packed.n_genomes
    dense = golden_dense(ctx, "jc", True)
    whole = dense.get("tree", list(range(n)))
    seed = (whole.source, whole.target, whole.weight)
    src, tgt, val, st = ctx.fill_rows_tree("jc", [], seed=seed, want_stats=True)             # n_rows == 0: the seeds come back
    assert np.array_equal(src, whole.source) and np.array_equal(tgt, whole.target) and same_bits(val, whole.weight) and st["n_slabs"] == 0
    for bad in ((whole.source, whole.target, whole.weight + 1e-9), (whole.source, whole.target, whole.weight + 1.0),
                (whole.target, whole.source, whole.weight), (whole.source, whole.target + n, whole.weight)):
        with pytest.raises(HipLibraryError, match="is no key"):
            ctx.fill_rows_tree("jc", [3], seed=bad)
    with pytest.raises(HipLibraryError, match="seed edges"):
        ctx.fill_rows_tree("jc", [3], seed=tuple(np.concatenate([x, x[:1]]) for x in seed))
    labels_whole = dense.get("components", list(range(n)), 0.75, True)
    labels, st = ctx.fill_rows_components("jc", 0.75, [], seed_labels=labels_whole, want_stats=True)
    assert np.array_equal(labels, labels_whole) and st["n_edges"] == 0 and st["n_slabs"] == 0
    assert np.array_equal(ctx.fill_rows_components("jc", 0.75, []), np.arange(n))             # no seed: every genome its own component
    for bad in (np.arange(n)[::-1], np.full(n, 1), np.r_[0, 0, 1, np.arange(3, n)]):
        with pytest.raises(HipLibraryError, match="seed_labels"):
            ctx.fill_rows_components("jc", 0.75, [3], seed_labels=bad.astype(np.int32))
    src, tgt, val = ctx.fill_rows_edges("jc", 0.75, [])
    assert src.shape == tgt.shape == val.shape == (0,)
    with pytest.raises(HipLibraryError, match="strictly ascending"):
        ctx.fill_rows_edges("jc", 0.75, [4, 4])
    # a seed that does not connect the old genomes: the existing refusal
    with pytest.raises(HipLibraryError, match="the forest holds"):
        ctx.fill_rows_tree("jc", [], seed=tuple(x[:-1] for x in seed))
    # the triangular calls still answer on this context
    got = ctx.fill_tree("jc")
    assert np.array_equal(got[0], whole.source) and same_bits(got[2], whole.weight)


# ---- 6: end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth200_genomes(native_built):
    from phamclust_amd.synth import synth_genomes
    return sorted(synth_genomes(2000, 5000), key=lambda g: g.name)[:200]


def test_extend_calls_equal_de_novo(synth200_genomes):
    from phamclust_amd import cli
    from phamclust_amd import matrix as M
    genomes, func = synth200_genomes, cli.METRICS["peq"]
    new = {3, 4, 60, 97, 131, 198, 199}
    old = [g for k, g in enumerate(genomes) if k not in new]
    tree, tree_old = M.tree_de_novo(genomes, func), M.tree_de_novo(old, func)
    got = M.tree_extend(tree_old, genomes, func)
    assert got.nodes == tree.nodes and np.array_equal(got.source, tree.source) and np.array_equal(got.target, tree.target)
    assert same_bits(got.weight, tree.weight) and got.is_distance
    assert M.LAST_FILL["rows"] == 7 and M.LAST_FILL["metric"] == "peq" and M.LAST_FILL["n_genomes"] == 200
    tampered = M.SingleLinkageTree(tree_old.nodes, tree_old.source, tree_old.target, tree_old.weight + np.r_[1e-6, np.zeros(len(tree_old) - 1)])
    with pytest.raises(ValueError, match="the tree holds"):
        M.tree_extend(tampered, genomes, func, verify=len(old))
    comps, comps_old = M.components_de_novo(genomes, func, 0.9), M.components_de_novo(old, func, 0.9)
    got = M.components_extend(comps_old, genomes, func, 0.9)
    assert got.nodes == comps.nodes and np.array_equal(got.labels, comps.labels)
    edges, edges_old = M.edges_de_novo(genomes, func, 0.9), M.edges_de_novo(old, func, 0.9)
    got = M.edges_extend(edges_old, genomes, func)
    assert got.nodes == edges.nodes and np.array_equal(got.source, edges.source) and np.array_equal(got.target, edges.target)
    assert same_bits(got.weight, edges.weight) and got.threshold == 0.9
    lacking = M.SparseEdges(edges_old.nodes, edges_old.source[1:], edges_old.target[1:], edges_old.weight[1:], threshold=0.9)
    with pytest.raises(ValueError, match="the edge list lacks it"):
        M.edges_extend(lacking, genomes, func, verify=len(old))
    with pytest.raises(ValueError, match="fill gives"):                      # another metric's file
        M.tree_extend(tree_old, genomes, cli.METRICS["jc"])


def test_cli_grow_reproduces_a_straight_run(synth200_genomes, tmp_path):
    from phamclust_amd.scripts import phamclust as script
    from phamclust_amd.synth import write_tsv
    genomes = synth200_genomes
    new = {3, 4, 60, 97, 131, 198, 199}
    all_tsv, old_tsv = tmp_path / "all.tsv", tmp_path / "old.tsv"
    write_tsv(genomes, all_tsv)
    write_tsv([g for k, g in enumerate(genomes) if k not in new], old_tsv)

    def run(name, tsv, *flags):
        out = tmp_path / name
        script.main([str(tsv), str(out), "-m", "jc", *flags])
        return out

    for flags, target in ((("--tree",), "tree_jc.tsv"), (("--components-only", "--edge-thresh", "0.1"), "components_jc.tsv")):
        tag = target.split("_")[0]
        straight = run(f"straight_{tag}", all_tsv, *flags)
        stored = run(f"old_{tag}", old_tsv, *flags)
        grown = run(f"grown_{tag}", all_tsv, *flags, "--grow", str(stored / target))
        assert (grown / target).read_bytes() == (straight / target).read_bytes()
        assert (stored / target).read_bytes() != (straight / target).read_bytes()
        log = (grown / "phamclust.log").read_text()
        assert "grown 193 -> 200 genomes: 7 rows, " in log and "pairs filled instead of 19,900" in log
