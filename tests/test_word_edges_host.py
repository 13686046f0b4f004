"""The word-edge collections of tests/word_edge_cases.py are the design they claim to be (CPU only).

tests/test_gpu_word_edges.py holds every bitmap-staging kernel to the oracle on these collections; that says something about the
32-word chunk edges only if the collections sit ON them and carry values there.  So, for every shape: the pham and word counts are
exact, every mark pham separates pairs, each extra genome shares phams inside its one word only, and the oracle's vectors spread."""

import numpy as np
import pytest

import word_edge_cases as WE


@pytest.mark.parametrize("shape", WE.SHAPES, ids=WE.shape_id)
def test_the_collection_is_the_design(native_built, shape):
    n_genomes, n_words, last_bits = shape
    packed = WE.collection(shape)
    P = WE.n_phams(n_words, last_bits)
    rows = WE.rows_of(packed)
    assert (packed.n_genomes, packed.n_phams, packed.words_per_row) == (n_genomes, P, n_words)
    assert packed.pham_names == [f"p{p:05d}" for p in range(P)]                              # name order is id order, no pham unheld
    last = np.bitwise_or.reduce(rows[:, -1])
    assert int(last) == (1 << last_bits) - 1                                                  # the last word: exactly last_bits bits in use
    # marks: both sides of every boundary the shape reaches, the first and the last pham
    mark = WE.marks(n_words, last_bits)
    assert {0, P - 1} <= set(mark)
    for b in WE.BOUNDARIES:
        want = [p for p in (64 * b - 65, 64 * b - 64, 64 * b - 1, 64 * b, 64 * b + 63) if p < P]
        assert set(want) <= set(mark)
        if n_words > b:
            assert len(want) >= 4                                                             # the boundary is crossed: marks on both sides
    for p in mark:
        holders = int(WE.holds(packed, p).sum())
        assert holders >= 2 and holders < n_genomes, (p, holders)                             # shared by a pair; held by one side of a pair
        assert 0.35 * n_genomes <= holders <= 0.85 * n_genomes, (p, holders)
    # the extras: all phams in one word, and a pair that shares something -- necessarily inside that word
    special = WE.extras(n_genomes, n_words)
    assert len(special) == (2 if n_words > WE.CHUNK else 1) and len({g for g, _ in special}) == len(special)
    for g, w in special:
        assert rows[g, w] != 0 and not np.delete(rows[g], w).any(), (g, w)
        shared = rows & rows[g]
        partners = [k for k in range(n_genomes) if k != g and shared[k].any()]
        assert partners and all(not np.delete(shared[k], w).any() for k in partners), (g, w)
        regular = [k for k in partners if k not in {x for x, _ in special}]
        assert regular and (n_words == 1 or any(np.delete(rows[k], w).any() for k in regular))                # ... with a genome that has phams elsewhere
    # paralogs and byte-identical translations exist
    assert (packed.ngen > packed.nph).sum() >= n_genomes // 2
    lens = np.diff(packed.seq_off)
    assert lens.min() >= 1 and lens.max() <= 30
    res = packed.residues.tobytes()
    assert len({res[int(a):int(b)] for a, b in zip(packed.seq_off[:-1], packed.seq_off[1:])}) <= 40
    # the oracle's vectors spread
    for metric in WE.SEVEN:
        for as_distance in (True, False):
            v = WE.oracle_fill(shape, metric, as_distance)
            assert v.shape == (packed.n_pairs,) and np.unique(v).size > 1, (metric, as_distance)
            if metric in ("jc", "af", "aai"):
                assert np.unique(v).size >= (5 if n_words == 1 else 20), (metric, as_distance, np.unique(v).size)
    assert WE.oracle_fill(shape, "jc", True) is WE.oracle_fill(shape, "jc", True)             # computed once


def test_the_shapes_cover_the_chunk_edges():
    """One word; one word short of a chunk, a chunk, a chunk and one bit; two chunks, two and a bit; three and a bit."""
    words = {w for _, w, _ in WE.SHAPES}
    assert {1, WE.CHUNK - 1, WE.CHUNK, WE.CHUNK + 1, 2 * WE.CHUNK, 2 * WE.CHUNK + 1, 3 * WE.CHUNK + 1} <= words
    assert {(w, b) for _, w, b in WE.SHAPES if w % WE.CHUNK == 1 and w > 1} == {(33, 1), (65, 1), (97, 1)}     # a final chunk of ONE pham
    assert any(w % 2 == 0 for w in words) and any(w % 2 == 1 and w > 1 for w in words)        # with and without the padding word of W | 1
    assert {n for n, _, _ in WE.SHAPES} == {33, 65}
    for shape in WE.SHAPES:
        n = shape[0]
        for rows in WE.row_sets(shape).values():
            assert rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < n
        families = WE.group_families(shape)
        for groups in families.values():
            for group in groups:
                assert group == sorted(set(group)) and 0 <= group[0] and group[-1] < n
        cuts = np.cumsum([len(g) for g in families["cut at 31, 32, 33"]]).tolist()
        assert cuts[:3] == [31, 32, 33]
        a, b = families["overlapping"]
        assert set(a) & set(b) and set(a) - set(b) and set(b) - set(a)
        assert {g for g, _ in WE.extras(n, shape[1])} <= set(families["extras + 3"][0]) and len(families["extras + 3"][0]) == len(WE.extras(n, shape[1])) + 3
