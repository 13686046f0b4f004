"""Designed collections with an EXACT bitmap word count, for the kernels that stage the presence bitmap 32 words at a time (no GPU
call here).

The popcount tiles (pc_set_popc.hip) and the three walkers (pc_walk.hip) stage 32 bitmap words per chunk; the walkers keep one bit
per staged word in a 32-bit mask, the word-split popcount tile deals a chunk's words to its four waves, and the device row stride is
W | 1.  `synth_packed` and `uniform_packed` number only the phams they happen to use, so neither can put a collection ON a chunk
edge.  `word_edge_packed` can: exactly 64 (n_words - 1) + last_bits phams, every one held, with
  * MARK phams on both sides of every chunk boundary (bits 0 and 63 of the words around it), of the first and of the last word,
    each held by ~60 % of the genomes -- a kernel that loses bit 63 of a chunk's last word, bit 0 of the next chunk's first, or the
    whole final chunk gets almost every pair wrong;
  * two EXTRA genomes whose phams all lie in one word -- the last word, and word 32 (the first word of the second chunk) --, so
    that what they share with anybody is found inside that staged chunk or not at all;
  * paralogs (pocp's second direction, aai's best-match loops) and translations from a small pool (byte-identical proteins, ties).
tests/test_word_edges_host.py proves on the CPU that every shape below is that design; tests/test_gpu_word_edges.py runs the kernels.
"""

import numpy as np

# (n_genomes, n_words, last_bits): one word; one short of a chunk; a chunk exactly; a chunk and one bit (the second chunk is ONE
# word holding ONE pham, and W | 1 == W: no padding word); two chunks exactly; two and one bit; three and one bit; and the
# 33-word case again with 33 genomes (one past the 32-pair tile only).  65 genomes cross the 32- and the 64-pair tile edge.
SHAPES = ((65, 1, 64), (65, 31, 63), (65, 32, 64), (65, 33, 1), (65, 64, 64), (65, 65, 1), (65, 97, 1), (33, 33, 1))
SEED = 20
CHUNK = 32                                   # bitmap words per staged chunk (WCH in pc_walk.hip, PWCH in pc_set_popc.hip)
BOUNDARIES = (32, 64, 96)
LETTERS = "ACDEFGHIKLMNPQRSTVWY"
SEVEN = ("gcs", "jc", "pocp", "af", "aai", "peq", "aai_ppos")


def shape_id(shape):
    return "{}x{}w{}b".format(*shape)


def n_phams(n_words, last_bits):
    return 64 * (n_words - 1) + last_bits


def marks(n_words, last_bits):
    """The mark phams of a shape, ascending: 0, P - 1 and, for each chunk boundary b the collection reaches, bits 63 of word b - 2,
    0 and 63 of word b - 1, 0 and 63 of word b -- those of them that exist."""
    P = n_phams(n_words, last_bits)
    out = {0, P - 1}
    for b in BOUNDARIES:
        out |= {64 * b - 65, 64 * b - 64, 64 * b - 1, 64 * b, 64 * b + 63}
    return sorted(p for p in out if 0 <= p < P)


def extras(n_genomes, n_words):
    """[(genome index, word)] of the extra genomes: all phams of genome 7 lie in the last word, all phams of genome n - 3 in word
    32 (where there is one; otherwise genome n - 3 is a regular genome).  With 33 words the two words are the same one."""
    out = [(7, n_words - 1)]
    if n_words > CHUNK:
        out.append((n_genomes - 3, CHUNK))
    return out


def word_range(word, n_words, last_bits):
    return range(64 * word, min(64 * word + 64, n_phams(n_words, last_bits)))


def _held_sets(n_genomes, n_words, last_bits, rng):
    P = n_phams(n_words, last_bits)
    mark = marks(n_words, last_bits)
    special = dict(extras(n_genomes, n_words))
    per = 90 if P > 128 else max(1, P // 2)
    held = [set() for _ in range(n_genomes)]
    regular = [g for g in range(n_genomes) if g not in special]
    for g in regular:
        held[g] = set(int(p) for p in rng.choice(P, size=min(P, int(per + rng.integers(-8, 9))), replace=False)) - set(mark)
        held[g] |= set(p for p in mark if rng.random() < 0.6)
    for p in range(P):                                                       # every pham has a holder
        if not any(p in held[g] for g in regular):
            held[regular[int(rng.integers(len(regular)))]].add(p)
    for g, w in special.items():
        own = list(word_range(w, n_words, last_bits))
        held[g] = set(int(p) for p in rng.choice(own, size=max(1, len(own) // 3), replace=False)) | (set(own) & set(mark))
    return held


def word_edge_packed(n_genomes, n_words, last_bits, seed=SEED):
    """`n_genomes` genomes (the extras among them) over exactly 64 (n_words - 1) + last_bits phams named p00000 ... (name order
    is id order), built through Genome + pack_genomes.  Deterministic in its arguments."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    rng = np.random.default_rng([seed, n_genomes, n_words, last_bits])
    pool = ["".join(LETTERS[int(c)] for c in rng.integers(0, 20, size=int(rng.integers(1, 31)))) for _ in range(40)]
    held = _held_sets(n_genomes, n_words, last_bits, rng)
    genomes = []
    for k in range(n_genomes):
        g = Genome(f"w{k:04d}")
        for p in sorted(held[k]):
            for _ in range(3 if rng.integers(11) == 0 else 1):               # one entry in eleven: a paralog with 3 copies
                g.add(f"p{p:05d}", pool[int(rng.integers(len(pool)))])
        genomes.append(g)
    return pack_genomes(genomes)


_built = {}


def collection(shape):
    """The packed collection of a shape, built once per process."""
    if shape not in _built:
        _built[shape] = word_edge_packed(*shape)
    return _built[shape]


def rows_of(packed):
    """The bitmap as an (N, W) uint64 array."""
    return packed.bitmap.reshape(packed.n_genomes, packed.words_per_row)


def holds(packed, pham):
    """Which genomes hold pham id `pham` (bool[N])."""
    return ((rows_of(packed)[:, pham >> 6] >> np.uint64(pham & 63)) & np.uint64(1)).astype(bool)


_oracle = {}


def oracle_fill(shape, metric, as_distance):
    """The oracle's whole condensed vector of a shape's collection, computed once per (shape, metric, polarity), read-only."""
    from oracle import oracle as O
    key = (shape, metric, bool(as_distance))
    if key not in _oracle:
        _oracle[key] = np.asarray(O.fill(collection(shape), metric, as_distance))
        _oracle[key].flags.writeable = False
    return _oracle[key]


def square(condensed, n, as_distance):
    """The full matrix of a condensed vector, the diagonal as matrix_de_novo presets it (tests/test_gpu_rows.square)."""
    full = np.zeros((n, n))
    s, t = np.triu_indices(n, k=1)
    full[s, t] = full[t, s] = np.asarray(condensed)
    np.fill_diagonal(full, 1.0 - as_distance)
    return full


# ---- the row sets and group families the GPU module runs ------------------------------------------------------------------
def row_sets(shape):
    n_genomes, n_words, _ = shape
    n = n_genomes
    rng = np.random.default_rng(n + n_words)
    per_tile = sorted(int(rng.integers(a, min(a + 32, n))) for a in range(0, n, 32))
    return {"first": [0], "last": [n - 1], "tile edge": [g for g in (31, 32, 33) if g < n], "one per tile": per_tile,
            "extras": sorted(g for g, _ in extras(n_genomes, n_words)), "all": list(range(n))}


def group_families(shape):
    """Families of groups over a shape's genomes: everything; groups whose boundaries fall on positions 31, 32 and 33 of the
    concatenated members; forty random pairs; two overlapping groups; the extras with three others."""
    n_genomes, n_words, _ = shape
    n = n_genomes
    rng = np.random.default_rng(1000 + n + n_words)
    pick = lambda size: sorted(rng.choice(n, size, replace=False).tolist())               # noqa: E731
    special = sorted(g for g, _ in extras(n_genomes, n_words))
    others = [g for g in (0, n // 2, n - 1) if g not in special]
    return {"everything": [list(range(n))],
            "cut at 31, 32, 33": [pick(31), pick(1), pick(1), pick(min(n, 40))],         # group_off = 0, 31, 32, 33, 73
            "forty pairs": [pick(2) for _ in range(40)],
            "overlapping": [list(range(2, 28)), list(range(20, n, 2))],
            "extras + 3": [sorted(special + others)]}


def condensed_of(full, group):
    """The condensed vector (scipy order) of the block of `full` over `group`."""
    group = np.asarray(group, dtype=np.int64)
    i, j = np.triu_indices(len(group), k=1)
    return full[group[i], group[j]]
