"""Value triangles and rows slabs for the distribution fill and the plain statement of its result (no GPU, no use of the library).

The triangles are tests/slab_value_cases.py's (target-major, element ``t (t - 1) / 2 + s`` the pair ``(s, t)``); the generators here are
the ones a histogram can go wrong on: one value everywhere (64 lanes on one address; the empty marker against key 0), values that all
differ (more keys per chunk than the workgroup's table has slots), and keys that share one probe run of the table.  ``hist`` is the
reference: ``np.bincount`` over int64 millionths.  tests/test_distribution_host.py holds it to ``PairDistribution.from_dense``;
tests/hist_values_driver.py holds the kernels to it."""

import numpy as np

import slab_value_cases as tri

MILLION = tri.MILLION
BINS = MILLION + 1
CHUNK = 4096                           # elements one workgroup of the pass covers (SLAB_CHUNK)
HASH = 2654435761                      # the table's hash: slot = (key * HASH mod 2^32) >> (32 - log2(slots)), as the C header states it
BAD_VALUES = (float("nan"), 1.0000005, -1e-6, 2.0, 0.1234565)


def slot_of(key, slots):
    """The first slot of ``key = cls << 20 | micro`` in a table of ``slots`` (a power of two)."""
    bits = int(slots).bit_length() - 1
    assert 1 << bits == int(slots)
    return ((int(key) * HASH) & 0xFFFFFFFF) >> (32 - bits)


# ---- generators ----------------------------------------------------------------------------------------------------------------
def constant(n, value):
    return np.full(tri.n_pairs(n), value, dtype=np.float64)


def rotation(n, micros):
    """Element i holds micros[i % len(micros)]: two values alternate lane by lane, 65 values shift by one lane per wave."""
    micros = np.asarray(micros, dtype=np.int64)
    return tri.of_micros(micros[np.arange(tri.n_pairs(n)) % micros.shape[0]])


def all_distinct(n, descending=False):
    """Every pair another millionth, ascending or descending in element order (n_pairs(n) <= 10^6 + 1)."""
    pairs = tri.n_pairs(n)
    assert pairs <= BINS
    micro = np.arange(pairs, dtype=np.int64) * (MILLION // max(pairs - 1, 1))
    return tri.of_micros(micro[::-1] if descending else micro)


def colliding_micros(slots, how_many, cls=0):
    """``how_many`` millionths whose keys of class ``cls`` all start at ONE slot of the table (the slot most millionths share, so the
    choice does not depend on luck), ascending."""
    key = (np.arange(BINS, dtype=np.uint64) | np.uint64(cls << 20)) * np.uint64(HASH) & np.uint64(0xFFFFFFFF)
    slot = (key >> np.uint64(32 - (int(slots).bit_length() - 1))).astype(np.int64)
    busiest = int(np.argmax(np.bincount(slot, minlength=slots)))
    micros = np.flatnonzero(slot == busiest)[:how_many]
    assert micros.shape[0] == how_many and all(slot_of(int(m) | (cls << 20), slots) == busiest for m in micros)
    return micros.astype(np.int64)


def collide(n, slots, probes, seed):
    """A triangle over probes + 12 millionths of one probe run (the run is longer than the probe bound: the last 12 keys of a chunk
    find no slot), bins 0 and 10^6, in random order and with unequal frequencies."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([colliding_micros(slots, probes + 12), [0, MILLION]])
    weight = rng.integers(1, 6, size=pool.shape[0]).astype(np.float64)
    return tri.of_micros(rng.choice(pool, size=tri.n_pairs(n), p=weight / weight.sum()))


def with_bad(values, positions):
    """A copy with values the fill must refuse at ``positions``: NaN, 1.0000005, -1e-6, 2.0 and a value between two millionths, in turn."""
    out = np.array(values, dtype=np.float64, copy=True)
    for i, at in enumerate(positions):
        out[at] = BAD_VALUES[i % len(BAD_VALUES)]
    return out


def labelings(n):
    """Partitions of n genomes: round-robin, blocks, one group, all singletons -- (labels int32[n], number of groups)."""
    g = np.arange(n, dtype=np.int32)
    return {"round-robin 5": (g % 5, 5), "blocks of 32": (g // 32, (n + 31) // 32), "one group": (np.zeros(n, dtype=np.int32), 1), "singletons": (g, n)}


def by_class(n, group, within_micro, between_micro):
    """Within pairs all one value, between pairs all another: a within / between mix-up changes the result."""
    s, t = tri.pair_ends(n)
    return tri.of_micros(np.where(group[s] == group[t], within_micro, between_micro))


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def hist_of_pairs(s, t, values, group=None, as_distance=True):
    """int64 [classes, BINS] of the pairs (s[i], t[i]) with DISTANCE values[i]; with ``group`` class 0 the pairs inside a group.  A
    similarity histogram is the distance histogram reversed: every millionth's complement."""
    micro = tri.micros_of(values)
    if group is None:
        out = np.bincount(micro, minlength=BINS).astype(np.int64)[None, :]
    else:
        group = np.asarray(group)
        same = group[s] == group[t]
        out = np.stack([np.bincount(micro[same], minlength=BINS), np.bincount(micro[~same], minlength=BINS)]).astype(np.int64)
    return np.ascontiguousarray(out if as_distance else out[:, ::-1])


def hist(values, n, group=None, as_distance=True):
    """The distribution fill's result for a whole triangle."""
    s, t = tri.pair_ends(n)
    return hist_of_pairs(s, t, values, group, as_distance)


def hist_among(values, n, members, group=None, as_distance=True):
    """... over the pairs with both genomes in ``members`` (a boolean mask): what a stored histogram of those genomes holds."""
    s, t = tri.pair_ends(n)
    keep = members[s] & members[t]
    return hist_of_pairs(s[keep], t[keep], np.asarray(values)[keep], group, as_distance)


def within_pairs(group, members=None):
    """Sum over the groups of n_c (n_c - 1) / 2, over the genomes of ``members`` (default: all)."""
    group = np.asarray(group, dtype=np.int64)
    if members is not None:
        group = group[members]
    sizes = np.bincount(group) if group.size else np.zeros(1, dtype=np.int64)
    return int(sum(int(c) * (int(c) - 1) // 2 for c in sizes))
