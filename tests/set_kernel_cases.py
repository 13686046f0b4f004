"""The designed collections of tests/test_gpu_set_kernels.py and the host-side arithmetic around them (no GPU call here).

gcs / jc / pocp / af are filled by one of five kernel families; which one, and in which launch shape, follows from what the
selector reads off the upload and the shard (`pc_set_inputs`).  This module
  * names the collections as generator calls (`COLLECTIONS`), deterministic in their arguments,
  * recounts the selector's inputs from a `PackedGenomes` with numpy alone (`recount`, `block_entries`, `target_costs`,
    `owned_targets`) -- never by asking a context,
  * asks the library's two host functions (`Context.set_kernel_choice`, `Context.set_launch_shape`) what family and shape every
    (collection, metric, shard) gets (`predict`), and
  * reduces a prediction to its coverage class (`class_of`).
tests/test_host.py proves on the CPU that the cases reach every class a default process can reach; the GPU module holds every fill
to the prediction (`Context.last_set_launch`) and every value to the oracle.
"""

import numpy as np

SET_METRICS = ("gcs", "jc", "pocp", "af")
FAMILIES = ("popc", "sparse", "sparse64", "walker", "sparsecol")
N_CU = 256                                     # compute units of an MI355X: what the CPU tests assume for the grid sizing
WORLDS = (3, 8)
DEALS = (False, True)                          # boustrophedon, cost-balanced


# ---- collections ------------------------------------------------------------------------------------------------------
def uniform_packed(n_genomes, n_phams, per_genome, seed):
    """Every genome holds `per_genome` phams drawn uniformly from `n_phams`, one gene each, translations of 1 ... 39 residues.
    125 of 5,056: 3.1 phams shared per pair, and 64 x 125 = 8,000 entries per block of 64 targets -- more than the column
    kernel's LDS value table holds at 5,056 mask entries (7,231)."""
    from phamclust_amd.pack import PackedGenomes
    rng = np.random.default_rng(seed)
    N, K, P = int(n_genomes), int(per_genome), int(n_phams)
    pham = np.sort(np.argsort(rng.random((N, P)), axis=1)[:, :K].astype(np.int32), axis=1).reshape(-1)
    present, gene_pham = np.unique(pham, return_inverse=True)
    gene_pham = gene_pham.astype(np.int32)
    P = int(present.shape[0])
    W = max(1, (P + 63) // 64)
    lens = rng.integers(1, 40, size=N * K).astype(np.int64)
    genome = np.repeat(np.arange(N, dtype=np.int64), K)
    bitmap = np.zeros(N * W, dtype=np.uint64)
    np.bitwise_or.at(bitmap, genome * W + (gene_pham >> 6), np.uint64(1) << (gene_pham & 63).astype(np.uint64))
    seq_off = np.zeros(N * K + 1, dtype=np.int64)
    np.cumsum(lens, out=seq_off[1:])
    return PackedGenomes(names=[f"u{g:06d}" for g in range(N)], pham_names=[f"p{int(p):06d}" for p in present], n_genomes=N, n_phams=P,
                         words_per_row=W, bitmap=bitmap, nph=np.full(N, K, np.int32), ngen=np.full(N, K, np.int32),
                         tlen=lens.reshape(N, K).sum(axis=1).astype(np.int64), gene_off=np.arange(N + 1, dtype=np.int64) * K,
                         gene_pham=gene_pham, seq_off=seq_off, residues=np.full(int(seq_off[-1]), ord("M"), np.uint8)).validate()


def with_empty_translation(packed, gene):
    """The same collection with gene `gene` translated to the empty string (the reference's `len("")`: af's summed length of
    that entry loses the gene's residues, metrics.py:135-147)."""
    import dataclasses
    lens = np.diff(packed.seq_off)
    a, b = int(packed.seq_off[gene]), int(packed.seq_off[gene + 1])
    lens[gene] = 0
    seq_off = np.zeros_like(packed.seq_off)
    np.cumsum(lens, out=seq_off[1:])
    tlen = packed.tlen.copy()
    tlen[int(np.searchsorted(packed.gene_off, gene, side="right")) - 1] -= b - a
    return dataclasses.replace(packed, seq_off=seq_off, tlen=tlen, residues=np.concatenate([packed.residues[:a], packed.residues[b:]]),
                               _keepalive=[]).validate()


def two_holder_case(rng, n_genomes, per_genome, wide=None, extra_holders=0):
    """Every pham of the pool is held by exactly two genomes (then `extra_holders` random ones get a third ... holder), so the dense
    pham count is the pool size n_genomes * per_genome / 2 -- whatever the vocabulary; `wide` = (genome, entries) gets a long row."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    pool = n_genomes * per_genome // 2
    slots = np.repeat(np.arange(pool), 2)
    rng.shuffle(slots)
    held = [set() for _ in range(n_genomes)]
    for k, p in enumerate(slots):                           # deal the shuffled (pham, pham) list round: a genome rarely gets both copies
        g = k % n_genomes
        if int(p) in held[g]:
            g = (g + 1) % n_genomes
        held[g].add(int(p))
    for p in rng.choice(pool, size=extra_holders, replace=False):
        for g in rng.choice(n_genomes, size=int(rng.integers(3, 40)), replace=False):
            held[int(g)].add(int(p))                        # phams with many holders: masks with many bits (broadcast adds)
    if wide is not None:
        held[wide[0]] |= set(int(x) for x in rng.choice(pool, size=wide[1], replace=False))
    genomes = []
    for k in range(n_genomes):
        g = Genome(f"g{k:04d}")
        for p in sorted(held[k]):
            for _ in range(int(rng.integers(2, 5)) if p % 7 == 0 else 1):      # paralogs: pocp's second direction
                g.add(f"p{p:05d}", "M" * int(rng.integers(1, 40)))
        g.add(f"own{k:04d}", "MK")                          # a pham nobody else holds: dropped from the dense numbering
        genomes.append(g)
    return pack_genomes(genomes)


# ---- the numeric-edge collection (tests/golden/set_edges/: the live reference's values for its 36 pairs) --------------------------
EDGE_NAMES = ("e0_copies65535", "e1_copies65536", "e2_phams1447", "e3_phams1448", "e4_genes1023", "e5_genes1024", "e6_entry65535",
              "e7_entry65536", "e8_empty")
# subsets that sit on one side of a guard each (the guards read the COLLECTION's maxima): name -> genomes
EDGE_SUBSETS = {
    "all": EDGE_NAMES,
    "lo": ("e0_copies65535", "e2_phams1447", "e4_genes1023", "e6_entry65535"),        # 65,535 genes, 1,447 phams, an entry of 65,535 residues
    "hi": ("e1_copies65536", "e3_phams1448", "e5_genes1024", "e7_entry65536"),        # one past each
    "genes1023": ("e4_genes1023", "e6_entry65535", "e8_empty"),                       # pocp's epilogue table: (2 x 1,023 + 1)^2 entries fit 4 Mi
    "genes1024": ("e4_genes1023", "e5_genes1024", "e6_entry65535"),                   # ... (2 x 1,024 + 1)^2 do not
    "phams1447": ("e2_phams1447", "e4_genes1023", "e6_entry65535"),                   # gcs / jc: 1,448 x 2,895 entries fit
    "phams1448": ("e2_phams1447", "e3_phams1448", "e5_genes1024"),                    # ... 1,449 x 2,897 do not
    "empty": ("e2_phams1447", "e4_genes1023", "e8_empty"),
}


def edge_genomes():
    """Nine genomes that sit on the selector's numeric guards and the epilogue table's limit, as Genome objects in name order:
    65,535 / 65,536 copies of one pham, 1,447 / 1,448 distinct phams, 1,023 / 1,024 genes, an entry of summed length
    65,535 / 65,536, and empty translations.  They share phams p0000 ... so that every pair has a value to get wrong."""
    from phamclust_amd.genome import Genome
    out = []
    for k, copies in enumerate((65535, 65536)):
        g = Genome(EDGE_NAMES[k])
        for _ in range(copies):
            g.add("p0000", "M")
        out.append(g)
    for k, phams in enumerate((1447, 1448)):
        g = Genome(EDGE_NAMES[2 + k])
        for p in range(phams):
            g.add(f"p{p:04d}", "MK" + "T" * (p % 3 + k))
        out.append(g)
    for k, genes in enumerate((1023, 1024)):
        g = Genome(EDGE_NAMES[4 + k])
        for j in range(genes):
            g.add(f"p{j % 100:04d}", "M" * (1 + (j + k) % 5))
        out.append(g)
    g = Genome(EDGE_NAMES[6])
    g.add("p0001", "M" * 65535)
    g.add("p0002", "MK")
    out.append(g)
    g = Genome(EDGE_NAMES[7])
    g.add("p0001", "M" * 32768)
    g.add("p0001", "K" * 32768)
    g.add("p0002", "M")
    out.append(g)
    g = Genome(EDGE_NAMES[8])
    g.add("p0000", "")
    g.add("p0001", "MKV")
    g.add("p0003", "")
    g.add("p0003", "MA")
    out.append(g)
    return out


def edge_packed(subset="all"):
    from phamclust_amd.pack import pack_genomes
    keep = set(EDGE_SUBSETS[subset])
    return pack_genomes([g for g in edge_genomes() if g.name in keep])


def edge_digest(genomes):
    """sha256 over the collection as (genome, pham, translation) rows in insertion order -- what tests/golden/set_edges/manifest.json
    records of the input the live reference was given (a TSV cannot carry an empty translation: the reference's loader reads a
    two-column row as "M", scripts/phamclust.py:35-38, so the fixture hands it Genome objects)."""
    import hashlib
    h = hashlib.sha256()
    for g in genomes:
        for pham, translations in g.phams.items():
            for t in translations:
                h.update(f"{g.name}\t{pham}\t{t}\n".encode())
    return h.hexdigest()


def sub_condensed(full, names, keep):
    """Condensed vector over the genomes `keep` (name order) out of the condensed vector `full` over `names`."""
    idx = [names.index(k) for k in keep]
    n = len(names)
    return np.array([full[a * n - a * (a + 1) // 2 + (b - a - 1)] for i, a in enumerate(idx) for b in idx[i + 1:]])


def _synth(n, p):
    from phamclust_amd.synth import synth_packed
    return synth_packed(n, p)


def _synth_real(n):
    from phamclust_amd.synth import synth_real
    return synth_real(n)


def _first_gene_of(packed, genome):
    return int(packed.gene_off[genome])


def _emptied(build, genome):
    return lambda: (lambda p: with_empty_translation(p, _first_gene_of(p, genome)))(build())


# name -> builder.  The collections of tests/test_gpu_set_kernels.py, then "synth20000" and "real1000": those of
# test_column_kernel_at_20000_genomes / test_full_size_set_metrics_vs_oracle and of test_real_collection_shape_full_matrix
# (tests/test_gpu_parity.py), which the coverage test counts in.
#   few*      synth(N, 1200): 19 bitmap words, 8.4 phams shared per pair -- the popcount tiles for gcs / jc / pocp, sparse64 for af
#   many*     synth(N, 10000 / 20000): more phams than the column kernel's masks hold -- sparse64's chunked instances from 3,000 genomes
#   col*      synth(N, 5000): the column kernel for all four
#   real*     synth_real(N): ~5.6 N phams, 4.4 N of them with two holders
#   uniform*  125 of 5,056 phams per genome: blocks of 8,000 entries overflow the column kernel's value table (pocp / af leave it)
#   *_empty   one gene translated to "": af leaves sparse64 for the 32 x 32 sparse tiles / the walker
COLLECTIONS = {
    "few400_empty": _emptied(lambda: _synth(400, 1200), 77),
    "few1000_empty": _emptied(lambda: _synth(1000, 1200), 500),
    "few1800_empty": _emptied(lambda: _synth(1800, 1200), 3),
    "few2999_empty": _emptied(lambda: _synth(2999, 1200), 2998),
    "few3600": lambda: _synth(3600, 1200),
    "few3600_empty": _emptied(lambda: _synth(3600, 1200), 1777),
    "few5000_empty": _emptied(lambda: _synth(5000, 1200), 4000),
    "few6400": lambda: _synth(6400, 1200),
    "few6400_empty": _emptied(lambda: _synth(6400, 1200), 0),
    "few12000": lambda: _synth(12000, 1200),
    "few20000": lambda: _synth(20000, 1200),
    "wide150_empty": _emptied(lambda: uniform_packed(150, 40000, 100, seed=3), 149),      # ~12,500 phams: more than one mask chunk of the 32 x 32 tiles
    "many1000_empty": _emptied(lambda: _synth(1000, 20000), 999),
    "many5000_empty": _emptied(lambda: _synth(5000, 20000), 2500),
    "many2600": lambda: _synth(2600, 10000),
    "many3600": lambda: _synth(3600, 10000),
    "many8192": lambda: _synth(8192, 10000),
    "many12000": lambda: _synth(12000, 10000),
    "many20000": lambda: _synth(20000, 10000),
    "twoholder160": lambda: two_holder_case(np.random.default_rng(160), 160, 100),
    "real1000_empty": _emptied(lambda: _synth_real(1000), 10),
    "real2000_empty": _emptied(lambda: _synth_real(2000), 1999),
    "real3000_empty": _emptied(lambda: _synth_real(3000), 1500),
    "real2000": lambda: _synth_real(2000),
    "real3000": lambda: _synth_real(3000),
    "uniform2300": lambda: uniform_packed(2300, 5056, 125, seed=5),
    "uniform2600": lambda: uniform_packed(2600, 5056, 125, seed=6),
    "uniform3600": lambda: uniform_packed(3600, 5056, 125, seed=8),
    "uniform4000": lambda: uniform_packed(4000, 5056, 125, seed=9),
    "uniform6000": lambda: uniform_packed(6000, 5056, 125, seed=7),
    "col2500": lambda: _synth(2500, 5000),
    "col4100": lambda: _synth(4100, 5000),
    "col7200": lambda: _synth(7200, 5000),
    "synth20000": lambda: _synth(20000, 5000),
    "real1000": lambda: _synth_real(1000),
}
# The unforced fills of tests/test_gpu_set_kernels.py: name -> (metrics, worlds sharded over -- every rank, both deals --, oracle).
# oracle "whole": every value of both polarities against O.fill; "sample": 200,000 pairs of both polarities against O.pairs and the
# whole matrix against a second, forced family.
AF, VALUES = ("af",), ("pocp", "af")
CASES = {
    "few400_empty": (SET_METRICS, WORLDS, "whole"), "few1000_empty": (SET_METRICS, WORLDS, "whole"), "few1800_empty": (SET_METRICS, WORLDS, "whole"),
    "few2999_empty": (SET_METRICS, WORLDS, "whole"), "few3600": (SET_METRICS, WORLDS, "whole"), "few3600_empty": (AF, (), "whole"),
    "few5000_empty": (SET_METRICS, WORLDS, "sample"), "few6400": (SET_METRICS, WORLDS, "sample"), "few6400_empty": (AF, WORLDS, "sample"),
    "few12000": (SET_METRICS, WORLDS, "sample"), "few20000": (AF, (3,), "sample"), "many20000": (SET_METRICS, (3,), "sample"),     # (3-way shards at super-tile edge 16)
    "wide150_empty": (SET_METRICS, WORLDS, "whole"), "many1000_empty": (AF, WORLDS, "whole"), "many5000_empty": (AF, WORLDS, "sample"),
    "many2600": (SET_METRICS, (), "sample"), "many3600": (SET_METRICS, (2,), "sample"), "many8192": (SET_METRICS, WORLDS, "sample"),
    "many12000": (SET_METRICS, WORLDS, "sample"), "twoholder160": (SET_METRICS, (), "whole"),
    "real1000_empty": (AF, WORLDS, "whole"), "real2000_empty": (AF, WORLDS, "whole"), "real3000_empty": (AF, WORLDS, "whole"),
    "real2000": (SET_METRICS, WORLDS, "whole"), "real3000": (SET_METRICS, WORLDS, "whole"),
    "uniform2300": (SET_METRICS, WORLDS, "whole"), "uniform2600": (VALUES, (), "whole"), "uniform3600": (VALUES, (2,), "sample"),
    "uniform4000": (VALUES, (2,), "sample"), "uniform6000": (SET_METRICS, WORLDS, "sample"),
    "col2500": (SET_METRICS, (), "whole"), "col4100": (SET_METRICS, WORLDS, "whole"), "col7200": (SET_METRICS, WORLDS, "sample"),
}
# The family each collection's UNSHARDED fill runs on, (gcs, jc, pocp, af), stated from pc_set_shape.hip's rules and the collections' profiles --
# few*: 19 words against 113 / 28 / 40 + a multiple of 8.4 shared: popcount tiles, af on sparse64 (with an empty translation: 32 x 32 tiles
# up to 3,500^2 pairs, then the walker); many*: 157 / 313 words, masks beyond the column kernel: sparse64 from 3,000^2 (pocp 2,500^2);
# real*: 267 words at N = 3,000 (9,000,000 pairs: sparse64), 175 at 2,000 (popcount tiles); uniform*: gcs / jc on the column kernel, pocp / af
# off it (blocks of 8,000 entries), pocp on sparse64 from 2,500^2; col*: the column kernel for all four.  The CPU coverage test holds the
# library's choice function to it, the GPU module every fill.
EXPECTED_WHOLE = {
    "few400_empty": ("popc", "popc", "popc", "sparse"),
    "few1000_empty": ("popc", "popc", "popc", "sparse"),
    "few1800_empty": ("popc", "popc", "popc", "sparse"),
    "few2999_empty": ("popc", "popc", "popc", "sparse"),
    "few3600": ("popc", "popc", "popc", "sparse64"),
    "few3600_empty": ("popc", "popc", "popc", "walker"),
    "few5000_empty": ("popc", "popc", "popc", "walker"),
    "few6400": ("popc", "popc", "popc", "sparse64"),
    "few6400_empty": ("popc", "popc", "popc", "walker"),
    "few12000": ("popc", "popc", "popc", "sparse64"),
    "few20000": ("popc", "popc", "popc", "sparse64"),
    "wide150_empty": ("popc", "popc", "popc", "sparse"),
    "many1000_empty": ("popc", "popc", "popc", "sparse"),
    "many5000_empty": ("sparse64", "sparse64", "sparse64", "walker"),
    "many2600": ("popc", "popc", "sparse64", "sparse64"),
    "many3600": ("sparse64", "sparse64", "sparse64", "sparse64"),
    "many8192": ("sparse64", "sparse64", "sparse64", "sparse64"),
    "many12000": ("sparse64", "sparse64", "sparse64", "sparse64"),
    "many20000": ("sparse64", "sparse64", "sparse64", "sparse64"),
    "twoholder160": ("popc", "popc", "popc", "sparse64"),
    "real1000_empty": ("popc", "popc", "popc", "sparse"),
    "real2000_empty": ("popc", "popc", "popc", "sparse"),
    "real3000_empty": ("sparse64", "sparse64", "sparse64", "sparse"),
    "real2000": ("popc", "popc", "popc", "sparse64"),
    "real3000": ("sparse64", "sparse64", "sparse64", "sparse64"),
    "uniform2300": ("sparsecol", "sparsecol", "popc", "sparse64"),
    "uniform2600": ("sparsecol", "sparsecol", "sparse64", "sparse64"),
    "uniform3600": ("sparsecol", "sparsecol", "sparse64", "sparse64"),
    "uniform4000": ("sparsecol", "sparsecol", "sparse64", "sparse64"),
    "uniform6000": ("sparsecol", "sparsecol", "sparse64", "sparse64"),
    "col2500": ("sparsecol", "sparsecol", "sparsecol", "sparsecol"),
    "col4100": ("sparsecol", "sparsecol", "sparsecol", "sparsecol"),
    "col7200": ("sparsecol", "sparsecol", "sparsecol", "sparsecol"),
}
# what the existing tests fill without a forced family, unsharded
EXISTING_CASES = {"synth20000": (SET_METRICS, (), "sample"), "real1000": (SET_METRICS, (), "whole")}

_built = {}


def collection(name):
    """(packed, recount) of a named collection, built once per process."""
    if name not in _built:
        packed = COLLECTIONS[name]()
        _built[name] = (packed, recount(packed))
    return _built[name]


def forget(name=None):
    """Drop a built collection (they take up to a few hundred MB)."""
    if name is None:
        _built.clear()
    else:
        _built.pop(name, None)


# ---- recounts from the packed arrays ----------------------------------------------------------------------------------------
def entries(packed):
    """(genome, pham, gene count, summed translation length) of every (genome, pham) entry, in genome order."""
    G = packed.n_genes
    genome = np.repeat(np.arange(packed.n_genomes, dtype=np.int64), np.diff(packed.gene_off))
    pham = packed.gene_pham.astype(np.int64)
    first = np.ones(G, dtype=bool)
    first[1:] = (pham[1:] != pham[:-1]) | (genome[1:] != genome[:-1])
    start = np.flatnonzero(first)
    lens = np.diff(packed.seq_off)
    cnt = np.diff(np.append(start, G))
    return genome[start], pham[start], cnt, (np.add.reduceat(lens, start) if G else np.zeros(0, np.int64))


def recount(packed):
    """What the upload counts for the selector, from the packed arrays alone."""
    N = packed.n_genomes
    e_genome, e_pham, e_cnt, e_len = entries(packed)
    holders = np.bincount(e_pham, minlength=max(packed.n_phams, 1))
    inc = float(np.sum(holders.astype(np.float64) * np.maximum(holders - 1, 0)))            # (integers below 2^53: exact in any order)
    lens = np.diff(packed.seq_off)
    return {
        "n": N, "words": packed.words_per_row, "holders": holders,
        "two_holder": int((holders >= 2).sum()),
        "avg_shared": inc / (float(N) * float(N - 1)) if N > 1 else 0.0,
        "max_nph": int(packed.nph.max()), "max_ngen": int(packed.ngen.max()), "max_tlen": int(packed.tlen.max()),
        "min_gene_len": int(lens.min()) if lens.size else 0,
        "max_ent_len": int(e_len.max()) if e_len.size else 0,
        # a genome's entries of phams with at least two holders: what a block of targets lays into the column kernel's value table
        "sp_n": np.bincount(e_genome, weights=(holders[e_pham] >= 2), minlength=N).astype(np.int64),
    }


def shared_per_pair(packed, s_idx, t_idx):
    """Phams the genome pairs (s, t) share, from the bitmap (a spot check of `avg_shared`'s closed form)."""
    rows = packed.bitmap.reshape(packed.n_genomes, packed.words_per_row)
    both = rows[np.asarray(s_idx)] & rows[np.asarray(t_idx)]
    return np.unpackbits(both.view(np.uint8), axis=1).sum(axis=1)


def target_costs(packed):
    """DP cells behind each target genome t: sum over s < t and over their shared phams of (summed length in s) x (summed length
    in t) -- what the cost-balanced deal weighs (pc_target_costs)."""
    e_genome, e_pham, _, e_len = entries(packed)
    order = np.lexsort((e_genome, e_pham))
    g, p, ln = e_genome[order], e_pham[order], e_len[order].astype(object)
    cost = [0] * packed.n_genomes
    run, prev = 0, -1
    for k in range(len(g)):                                  # prefix sums within a pham, in genome order (exact Python integers)
        if p[k] != prev:
            run, prev = 0, p[k]
        cost[int(g[k])] += int(ln[k]) * run
        run += int(ln[k])
    return np.array(cost, dtype=np.uint64)


def owned_targets(packed, rank, world, balanced, costs=None):
    """Ascending target genomes rank `rank` of `world` owns under the boustrophedon or the cost-balanced deal."""
    from phamclust_amd import distributed as D
    if world == 1:
        return np.arange(packed.n_genomes, dtype=np.int64)
    if not balanced:
        return np.asarray(D.shard_targets(packed.n_genomes, rank, world), dtype=np.int64)
    t_rank, _, _ = D.balanced_deal(target_costs(packed) if costs is None else costs, world)
    return np.flatnonzero(np.asarray(t_rank) == rank).astype(np.int64)


def block_entries(stats, owned=None):
    """Entries (of phams with two holders) of every block of 64 consecutive owned targets, the last, ragged block included."""
    sp_n = stats["sp_n"] if owned is None else stats["sp_n"][np.asarray(owned, dtype=np.int64)]
    if sp_n.size == 0:
        return np.zeros(0, np.int64)
    return np.add.reduceat(sp_n, np.arange(0, sp_n.size, 64))


def selector_inputs(stats, owned=None):
    """The `pc_set_inputs` fields (without metric / forced) of a fill of that collection by the rank that owns `owned`."""
    blocks = block_entries(stats, owned)
    fields = {k: stats[k] for k in ("n", "words", "two_holder", "avg_shared", "max_nph", "max_ngen", "min_gene_len", "max_ent_len", "max_tlen")}
    fields["nown"] = stats["n"] if owned is None else int(len(owned))
    fields["max_block_entries"] = int(blocks.max()) if blocks.size else 0
    return fields


def predict(C, stats, metric, owned=None, forced=None, n_cu=N_CU, **knobs):
    """(selector inputs, family, launch shape) the library's host functions give that fill."""
    fields = selector_inputs(stats, owned)
    family = C.set_kernel_choice(metric, forced=forced, **fields)
    top = stats["max_ngen"] if metric == "pocp" else stats["max_nph"]
    shape = C.set_launch_shape(family, metric, fields["n"], fields["nown"], fields["words"], fields["two_holder"], n_cu=n_cu, table_top=top, **knobs)
    return fields, family, shape


# ---- coverage classes -------------------------------------------------------------------------------------------------------
CLASS_FIELDS = ("family", "metric group", "tile edge", "super-tile edge", "several units per workgroup / seg > 1", "mask chunks > 1",
                "instance (batches, dense)", "epilogue table", "sharded")


def metric_group(metric):
    return "counts" if metric in ("gcs", "jc") else metric


def class_of(metric, shape, sharded):
    several = shape["seg"] > 1 if shape["family"] == "sparsecol" else shape["units_per_wg"] > 1
    return (shape["family"], metric_group(metric), shape["tile"], shape["super_edge"], bool(several), shape["chunks"] > 1,
            (shape["batches"], shape["dense"]), shape["table"] if shape["family"] == "popc" else None, bool(sharded))


def class_name(cls):
    return ", ".join(f"{k}: {v}" for k, v in zip(CLASS_FIELDS, cls))


def shards_of(packed, worlds):
    """[(world, rank, balanced, owned)]: the unsharded fill, then every rank of `worlds` x DEALS."""
    shards = [(1, 0, False, None)]
    if worlds:
        costs = target_costs(packed)
        shards += [(w, r, b, owned_targets(packed, r, w, b, costs)) for w in worlds for b in DEALS for r in range(w)]
    return shards


def classes_by_case(C, cases):
    """{name: {class: (name, metric, world, rank, deal)}} over the unforced fills of `cases` (CASES / EXISTING_CASES entries)."""
    out = {}
    for name, (metrics, worlds, _) in cases.items():
        packed, stats = collection(name)
        reached = out.setdefault(name, {})
        for world, rank, balanced, owned in shards_of(packed, worlds):
            for metric in metrics:
                _, family, shape = predict(C, stats, metric, owned)
                if world == 1 and name in EXPECTED_WHOLE:
                    assert family == EXPECTED_WHOLE[name][SET_METRICS.index(metric)], (name, metric, family)
                reached.setdefault(class_of(metric, shape, world > 1), (name, metric, world, rank, "balanced" if balanced else "boustrophedon"))
        forget(name)
    return out


def union_classes(by_case, without=()):
    """{class: first case that reaches it}, leaving out the cases whose name starts with one of `without`."""
    reached = {}
    for name, classes in by_case.items():
        if not any(name.startswith(w) for w in without):
            for cls, case in classes.items():
                reached.setdefault(cls, case)
    return reached


# ---- what a default process can reach ------------------------------------------------------------------------------------------
# Collection profiles of the generators: (bitmap words, phams with two holders, phams an average pair shares).  synth(N, P): every
# pham has many holders (two_holder = P), shared falls from ~34 (P = 300) to ~0.4 (P = 40,000); synth_real(N): ~5.6 N phams,
# ~4.4 N of them with two holders, ~3.6 shared; the uniform draw: 5,056 phams, ~3.1 shared.
def sweep_profiles(n):
    out = [(max(1, (p + 63) // 64), p, shared) for p, shared in ((300, 34.0), (1200, 8.4), (2500, 5.0), (5000, 2.85), (5056, 3.1),
                                                                 (7872, 2.0), (10000, 1.4), (20000, 0.7), (40000, 0.36))]
    real_p = max(64, int(5.6 * n))
    return out + [((real_p + 63) // 64, max(1, int(4.4 * n)), 3.6)]


SWEEP_N = (2, 33, 65, 200, 400, 700, 1000, 1399, 1400, 1800, 2199, 2200, 2499, 2500, 2999, 3000, 3499, 3500, 3600, 3999, 4000, 4100, 5000,
           5999, 6000, 6400, 7200, 8000, 10000, 12000, 14000, 16000, 18000, 20000)
SWEEP_WORLDS = (1, 2, 3, 4, 8)
# the guards: what a collection can do to the selector beyond its size (each a dict of pc_set_inputs overrides)
SWEEP_GUARDS = ({}, {"min_gene_len": 0}, {"max_block_entries": 1 << 20})


def reachable_classes(C, n_values=SWEEP_N, worlds=SWEEP_WORLDS, n_cu=N_CU):
    """{class: one input that reaches it} over the sweep above: every N x world (nown = the boustrophedon share of rank 0) x
    profile x guard x metric, through the library's two host functions.  No forced family, no knob: a default process."""
    reachable = {}
    for n in n_values:
        for world in worlds:
            nown = n if world == 1 else max(1, n // world)
            for words, two_holder, shared in sweep_profiles(n):
                for guard in SWEEP_GUARDS:
                    fields = dict(n=n, nown=nown, words=words, two_holder=two_holder, avg_shared=shared, max_nph=140, max_ngen=160,
                                  min_gene_len=1, max_ent_len=3000, max_tlen=40000, max_block_entries=6500)
                    fields.update(guard)
                    for metric in SET_METRICS:
                        family = C.set_kernel_choice(metric, **fields)
                        top = fields["max_ngen"] if metric == "pocp" else fields["max_nph"]
                        shape = C.set_launch_shape(family, metric, n, nown, words, two_holder, n_cu=n_cu, table_top=top)
                        reachable.setdefault(class_of(metric, shape, world > 1), (metric, fields))
    return reachable
