"""The child process of tests/test_gpu_slab_values.py: ``python slab_values_driver.py <case>`` under PHAMCLUST_NATIVE_VARIANT=hooks and
PHAMCLUST_NO_TORCH=1 (the variant is chosen when phamclust_amd.hip is imported, so the cases cannot run inside pytest's process).

Every case uploads ``hand_built(n)`` -- n genomes that share no pham; the collection only sets N --, injects a value triangle of
tests/slab_value_cases.py through ``hip.set_slab_values`` and compares what a slab fill makes of it with the plain reference there,
exactly: ``np.array_equal`` on integers or on the uint64 view of values.  It asserts everything itself and ends with
``ok <case> <number of comparisons>``."""

import ctypes
import itertools
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import slab_value_cases as cases                                            # noqa: E402
from phamclust_amd import hip                                                # noqa: E402

METRIC = "jc"
MILLION = cases.MILLION
COMPARED = [0]


def same(got, want, label):
    """One exact comparison: dtype, shape and every element (floats by their bits)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float64:
        got, want = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    if not np.array_equal(got, want):
        first = np.argwhere(got != want)[0].tolist()
        raise AssertionError(f"{label}: {int((got != want).sum())} of {got.size} elements differ, the first at {first}: "
                             f"{got[tuple(first)]!r} for {want[tuple(first)]!r}")
    COMPARED[0] += 1


def truth(condition, label):
    assert condition, label
    COMPARED[0] += 1


def hand_built(n):
    """n genomes of four genes each that share no pham (the "disjoint" collection of tests/test_gpu_tree.py)."""
    from phamclust_amd.genome import Genome
    from phamclust_amd.pack import pack_genomes
    genomes = []
    for k in range(n):
        g = Genome(f"g{k:04d}")
        for j in range(4):
            g.add(f"p{k}_{j}", "MKTAYIAKQRQISFVKSHFSRQ"[: 12 + 3 * j])
        genomes.append(g)
    return pack_genomes(genomes)


def context(n):
    ctx = hip.Context(0)
    ctx.upload(hand_built(n), residues=False)
    return ctx


def n_slabs(n, slab_bytes):
    return len(hip.Context.edge_slabs(n, slab_bytes)) - 1 if slab_bytes else 1


def labelings(n):
    return {"g % 5": (np.arange(n, dtype=np.int32) % 5, 5), "blocks of 64": (np.arange(n, dtype=np.int32) // 64, (n + 63) // 64),
            "singletons": (np.arange(n, dtype=np.int32), n)}


THREE_SLABS = 8 * 3000                 # N = 130: targets [0, 77), [77, 109), [109, 130)


# ---- tree ----------------------------------------------------------------------------------------------------------------
def check_tree(ctx, values, n, label, slabs=(0,)):
    hip.set_slab_values(values)
    for as_distance in (True, False):
        want = cases.kruskal(values, n, as_distance)
        for slab_bytes in slabs:
            src, tgt, val, st = ctx.fill_tree(METRIC, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
            truth(st["n_slabs"] == n_slabs(n, slab_bytes) and st["n_edges"] == n - 1, (label, as_distance, slab_bytes, st["n_slabs"]))
            for got, stated, what in ((src, want[0], "src"), (tgt, want[1], "tgt"), (val, want[2], "val")):
                same(got, stated, (label, what, as_distance, slab_bytes))
    hip.set_slab_values(None)


def case_tree():
    n = 130
    assert n_slabs(n, 8 * 1000) >= 8
    with context(n) as ctx:
        for label, values in (("two_valued 0.02", cases.two_valued(n, 0.02, 11)), ("two_valued 0.5", cases.two_valued(n, 0.5, 12)),
                              ("two_valued 0.5 on 499999 / 500000", cases.rescaled(cases.two_valued(n, 0.5, 13), 499999, 500000)),
                              ("tie_set", cases.tie_set(n, 14)), ("ramp", cases.ramp(n))):
            check_tree(ctx, values, n, label, slabs=(0, 8 * 1000))


def case_tree_tiny():
    """N = 2 and 3 with every tie pattern: every assignment of three millionths to the pairs."""
    micros = (0, 500000, 1000000)
    with context(2) as ctx:
        for a in micros:
            check_tree(ctx, cases.of_micros([a]), 2, ("n = 2", a))
    with context(3) as ctx:
        for pattern in itertools.product(micros, repeat=3):
            check_tree(ctx, cases.of_micros(pattern), 3, ("n = 3", pattern), slabs=(0, 8))


# ---- components and edges ------------------------------------------------------------------------------------------------------
def check_threshold(ctx, values, n, threshold, as_distance, label, slab_bytes=0):
    """The edge fill and both components fills at one threshold (the hook is set)."""
    src, tgt, val, st = ctx.fill_edges(METRIC, threshold, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
    want = cases.edge_list(values, n, threshold, as_distance, strict=False)
    for got, stated, what in ((src, want[0], "src"), (tgt, want[1], "tgt"), (val, want[2], "val")):
        same(got, stated, (label, "edges", what))
    for strict in (True, False):
        labels, cst = ctx.fill_components(METRIC, threshold, as_distance=as_distance, strict=strict, slab_bytes=slab_bytes, want_stats=True)
        stated, n_pass = cases.components(values, n, threshold, as_distance, strict)
        same(labels, stated, (label, "labels", strict))
        truth(cst["n_edges"] == n_pass and cst["n_components"] == np.unique(stated).shape[0], (label, "counts", strict, cst["n_edges"], n_pass))
        if not strict:
            truth(cst["n_edges"] == st["n_edges"] == want[0].shape[0], (label, "the non-strict count is the edge fill's"))


def case_components_edges(n):
    with context(n) as ctx:
        for p in (0.5 / n, 1.0 / n, math.log(n) / n, 0.5):
            values = cases.two_valued(n, p, 21 + n)
            hip.set_slab_values(values)
            for as_distance in (True, False):
                for threshold in (5e-7, 0.0, 1e-6):                         # between the two values, and at each of them
                    check_threshold(ctx, values, n, threshold, as_distance, (n, p, as_distance, threshold))
            check_threshold(ctx, values, n, 5e-7, True, (n, p, "slabs"), slab_bytes=8 * (cases.n_pairs(n) // 5))
            hip.set_slab_values(None)


def case_components_edges_finite():
    n = 130
    values = cases.finite_doubles(n, 31)
    present = np.unique(values)
    picks = [present[0], present[present.shape[0] // 3], present[present.shape[0] // 2], 1.0, 5e-324, present[-1]]
    with context(n) as ctx:
        hip.set_slab_values(values)
        for as_distance in (True, False):
            for v in picks:
                truth(bool((values == v).any()), ("a present value", v))
                for threshold in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
                    if np.isfinite(threshold):
                        check_threshold(ctx, values, n, float(threshold), as_distance, ("finite", as_distance, float(threshold).hex()))
            for zero in (0.0, -0.0):
                check_threshold(ctx, values, n, zero, as_distance, ("finite", as_distance, zero), slab_bytes=THREE_SLABS)
        hip.set_slab_values(None)


# ---- nearest --------------------------------------------------------------------------------------------------------------
def case_nearest():
    n = 130
    assert n_slabs(n, THREE_SLABS) == 3
    with context(n) as ctx:
        for label, values in (("tie_set", cases.tie_set(n, 41)), ("two_valued", cases.two_valued(n, 0.5, 42)), ("finite_doubles", cases.finite_doubles(n, 43))):
            hip.set_slab_values(values)
            for as_distance in (True, False):
                want_nbr, want_val = cases.nearest(values, n, 64, as_distance)
                for k in (1, 63, 64):
                    for slab_bytes in (0, THREE_SLABS):
                        nbr, val, st = ctx.fill_nearest(METRIC, k, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
                        truth(st["k"] == k and st["n_slabs"] == n_slabs(n, slab_bytes), (label, k, st["n_slabs"]))
                        same(nbr, want_nbr[:, :k], (label, "nbr", as_distance, k, slab_bytes))
                        same(np.ascontiguousarray(val).view(np.uint64), want_val[:, :k], (label, "val", as_distance, k, slab_bytes))
            hip.set_slab_values(None)


# ---- between ---------------------------------------------------------------------------------------------------------------
def check_between(fill, values, n, group, n_groups, label, slabs=(0,)):
    for as_distance in (True, False):
        want = cases.between(values, n, group, n_groups, as_distance)
        for slab_bytes in slabs:
            got = fill(METRIC, group, n_groups, as_distance=as_distance, slab_bytes=slab_bytes)
            for arr, stated, what in zip(got, want, ("sum", "count", "lo", "hi")):
                same(arr, stated, (label, what, as_distance, slab_bytes))


def case_between():
    n = 515
    with context(n) as ctx:
        for name, values in (("ramp", cases.ramp(n)), ("tie_set", cases.tie_set(n, 51))):
            hip.set_slab_values(values)
            for label, (group, n_groups) in labelings(n).items():
                check_between(ctx.fill_between, values, n, group, n_groups, (name, label), slabs=(0, 8 * 40000))
            hip.set_slab_values(None)


def case_between_segment():
    n = hip.Context.between_segment() + 3                                   # the last rows are two segments long
    values = cases.ramp(n)
    with context(n) as ctx:
        hip.set_slab_values(values)
        check_between(ctx.fill_between, values, n, np.arange(n, dtype=np.int32) % 5, 5, "two segments")
        hip.set_slab_values(None)


# ---- affinity --------------------------------------------------------------------------------------------------------------
AFFINITY_KEYS = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")


def check_affinity(fill, values, n, group, n_groups, label, slabs=(0,), directions=(True, False)):
    for as_distance in directions:
        want = cases.affinity(values, n, group, n_groups, as_distance)
        for slab_bytes in slabs:
            got = fill(METRIC, group, n_groups, as_distance=as_distance, slab_bytes=slab_bytes, want_table=True)
            for key in AFFINITY_KEYS:
                same(got[key], want[key], (label, key, as_distance, slab_bytes))
            for arr, stated, what in zip(got["table"], want["table"], ("sum", "lo", "hi")):
                same(arr, stated, (label, "table " + what, as_distance, slab_bytes))
    return want


def case_affinity():
    for n in (65, 129):
        with context(n) as ctx:
            for name, values in (("ramp", cases.ramp(n)), ("tie_set", cases.tie_set(n, 61 + n))):
                hip.set_slab_values(values)
                for label, (group, n_groups) in labelings(n).items():
                    check_affinity(ctx.fill_affinity, values, n, group, n_groups, (n, name, label), slabs=(0, 8 * (cases.n_pairs(n) // 3)))
                hip.set_slab_values(None)


def case_affinity_mean_tie():
    """Two groups of different size whose sums to genome 0 are in the ratio of their sizes -- exactly equal means -- under group
    indices that put the two into one lane of k_aff_finish (indices 64 apart), into neighbouring lanes and into distant ones, the
    smaller group first and second: the tie goes to the smaller INDEX.  Every other group is farther from genome 0."""
    n, n_groups = 16, 130
    with context(n) as ctx:
        for to_a, to_b in (((300000, 100000), (100000, 200000, 300000)), ((200000,), (100000, 200000, 200000, 300000))):
            for index_a, index_b in ((3, 67), (67, 3), (3, 4), (4, 3), (70, 7), (7, 70), (0, 128), (128, 0)):
                full = cases.square(cases.tie_set(n, 71), n).copy()
                group = np.zeros(n, dtype=np.int32)
                group[0] = 129
                members_a = list(range(1, 1 + len(to_a)))
                members_b = list(range(1 + len(to_a), 1 + len(to_a) + len(to_b)))
                rest = [g for g in range(1, n) if g not in members_a + members_b]
                spare = [b for b in range(n_groups) if b not in (index_a, index_b, 129)]
                for g, micro in zip(members_a + members_b, to_a + to_b):
                    full[0, g] = full[g, 0] = micro / 1000000.0
                    group[g] = index_a if g in members_a else index_b
                for i, g in enumerate(rest):
                    full[0, g] = full[g, 0] = 0.9
                    group[g] = spare[(i * 17) % len(spare)]
                values = hip.triangle_of(full)
                hip.set_slab_values(values)
                want = check_affinity(ctx.fill_affinity, values, n, group, n_groups, ("mean tie", index_a, index_b, len(to_a)))
                truth(sum(to_a) * len(to_b) == sum(to_b) * len(to_a) and want["near_group"][0, 0] == min(index_a, index_b), ("the tie is there", index_a, index_b))
                hip.set_slab_values(None)


def case_affinity_ranges():
    """N = 2,049 in 600 near-equal groups: whatever the device's CU count (up to 512), every group range of the column pass holds at
    least two non-empty groups, so the loop over several groups in one wave runs everywhere."""
    n, n_groups = 2049, 600
    group = (np.arange(n, dtype=np.int32) * 7) % n_groups
    goff = cases.affinity_goff(group, n_groups)
    most = math.ceil(16 * 512 / math.ceil(n / hip.Context.affinity_block()))
    truth(most == 249 and (np.diff(goff) >= 3).all(), "the shape of the case")
    for want in range(1, most + 1):
        cut = hip.Context.affinity_ranges(goff, n, want)
        assert cut[0] == 0 and cut[-1] == n_groups and (np.diff(cut) >= 2).all(), (want, cut)
    COMPARED[0] += most
    values = cases.spread(n, 81)
    with context(n) as ctx:
        hip.set_slab_values(values)
        check_affinity(ctx.fill_affinity, values, n, group, n_groups, "multi-group ranges", slabs=(0, 8 * 700000), directions=(True,))
        hip.set_slab_values(None)


# ---- several devices --------------------------------------------------------------------------------------------------------
def case_multi():
    n = 130
    values = cases.tie_set(n, 91)
    packed = hand_built(n)
    group, n_groups = np.arange(n, dtype=np.int32) % 5, 5
    with hip.Context(0) as ctx, hip.MultiContext([0] * 3) as multi:
        ctx.upload(packed, residues=False)
        multi.upload(packed, residues=False)
        hip.set_slab_values(values)
        for as_distance in (True, False):
            label = ("multi", as_distance)
            for got, want in zip(multi.fill_edges(METRIC, 0.5, as_distance=as_distance, slab_bytes=8 * 1000), ctx.fill_edges(METRIC, 0.5, as_distance=as_distance)):
                same(got, want, label + ("edges",))
            same(multi.fill_edges(METRIC, 0.5, as_distance=as_distance)[2], cases.edge_list(values, n, 0.5, as_distance)[2], label + ("edges, stated",))
            for strict in (True, False):
                same(multi.fill_components(METRIC, 0.5, as_distance=as_distance, strict=strict, slab_bytes=8 * 1000),
                     ctx.fill_components(METRIC, 0.5, as_distance=as_distance, strict=strict), label + ("components", strict))
            for got, want in zip(multi.fill_nearest(METRIC, 64, as_distance=as_distance, slab_bytes=8 * 1000), ctx.fill_nearest(METRIC, 64, as_distance=as_distance)):
                same(got, want, label + ("nearest",))
            got = multi.fill_tree(METRIC, as_distance=as_distance, slab_bytes=8 * 1000)
            for arr, want, stated in zip(got, ctx.fill_tree(METRIC, as_distance=as_distance), cases.kruskal(values, n, as_distance)):
                same(arr, want, label + ("tree",))
                same(arr, stated, label + ("tree, stated",))
            for arr, want in zip(multi.fill_between(METRIC, group, n_groups, as_distance=as_distance, slab_bytes=8 * 1000), ctx.fill_between(METRIC, group, n_groups, as_distance=as_distance)):
                same(arr, want, label + ("between",))
            check_between(multi.fill_between, values, n, group, n_groups, label + ("between, stated",))
            got, want = (c.fill_affinity(METRIC, group, n_groups, as_distance=as_distance, want_table=True) for c in (multi, ctx))
            for key in AFFINITY_KEYS:
                same(got[key], want[key], label + ("affinity", key))
            for arr, stated in zip(got["table"], want["table"]):
                same(arr, stated, label + ("affinity table",))
        check_affinity(multi.fill_affinity, values, n, group, n_groups, ("multi", "affinity, stated"), slabs=(8 * 1000,))
        st = multi.fill_tree(METRIC, want_stats=True)[3]
        truth(st["n_devices"] == 3 and all(a < b for a, b in zip(st["stretches"], st["stretches"][1:])), ("three stretches with pairs", st["stretches"]))
        hip.set_slab_values(None)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
_i32p, _i64p, _f64p = hip._i32p, hip._i64p, hip._f64p


def raw_call(lib, handle, symbol, kinds, n_counts, args, stats):
    """A fill through the C-ABI -- ``kinds``: its output pointers, ``n_counts``: the int32 counts behind them --: (status, which output
    pointers are set, the error text)."""
    cells = [kind() for kind in kinds]
    counts = [ctypes.c_int32(7) for _ in range(n_counts)]
    rc = getattr(lib, symbol)(handle, hip.METRIC_IDS[METRIC], *args, *(ctypes.byref(c) for c in cells), *(ctypes.byref(c) for c in counts), stats)
    return rc, [bool(c) for c in cells], lib.pc_last_error().decode()


def refused_fills(owner, prefix, group, n_groups, slab_bytes):
    """{fill: (status, pointers, message)} of the three fills that check their values, through the C-ABI."""
    lib, handle = owner._lib, owner._h
    stats = (hip.PcStats * 3)()
    pgroup = group.ctypes.data_as(_i32p)
    return {
        "tree": raw_call(lib, handle, prefix + "tree", (_i32p, _i32p, _f64p), 2, (1, slab_bytes), stats),
        "between": raw_call(lib, handle, prefix + "between", (_i64p, _i64p, _i32p, _i32p), 1, (1, pgroup, n_groups, slab_bytes), stats),
        "affinity": raw_call(lib, handle, prefix + "affinity", (_i64p, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p, _i64p, _i32p, _i32p), 1,
                             (1, pgroup, n_groups, 1, slab_bytes), stats),
    }


def counted(message):
    found = re.search(r": (\d+) values of the fill are no millionth in \[0, 1\]", message)
    assert found, message
    return int(found.group(1))


def case_refusals():
    n = 130
    pairs = cases.n_pairs(n)
    cut = hip.Context.edge_slabs(n, THREE_SLABS).tolist()
    assert cut == [0, 77, 109, 130]
    odd_row = 58
    assert cases.pair_index(0, odd_row) % 2 == 1 and cases.pair_index(0, 57) % 2 == 0
    positions = [0, pairs - 1, cases.pair_index(0, 57), cases.pair_index(56, 57), cases.pair_index(0, odd_row),
                 cases.pair_index(20, 40), cases.pair_index(50, 90), cases.pair_index(100, 120)]      # the last three: one per slab
    assert len(set(positions)) == len(positions) and [sum(cut[i] <= t < cut[i + 1] for t in (40, 90, 120)) for i in range(3)] == [1, 1, 1]
    clean = cases.spread(n, 101)
    bad = cases.with_bad(clean, positions)
    group, n_groups = np.arange(n, dtype=np.int32) % 5, 5
    packed = hand_built(n)
    with hip.Context(0) as ctx, hip.MultiContext([0] * 3) as multi:
        ctx.upload(packed, residues=False)
        multi.upload(packed, residues=False)
        plain_fill = ctx.fill(METRIC)
        plain_affinity = ctx.fill_affinity(METRIC, group, n_groups, want_table=True)
        plain_multi = multi.fill_between(METRIC, group, n_groups)
        truth(ctx.shard_pairs() == pairs, "the unsharded context")
        hip.set_slab_values(bad)
        for owner, prefix in ((ctx, "pc_fill_"), (multi, "pc_multi_fill_")):
            for slab_bytes in (0, THREE_SLABS):
                for fill, (rc, pointers, message) in refused_fills(owner, prefix, group, n_groups, slab_bytes).items():
                    label = (prefix + fill, slab_bytes, message)
                    truth(rc == -5 and not any(pointers), label)
                    truth((prefix + fill) in message, label)
                    if fill == "tree":
                        truth(counted(message) >= 1, label)                   # sightings, not values: the count depends on the rounds
                    else:
                        truth(counted(message) == len(positions), label)
        # a refused walk leaves the context whole: the hook cleared, the plain fills are what they were
        hip.set_slab_values(None)
        truth(ctx.shard_pairs() == pairs, "the unsharded context, after the refusals")
        same(ctx.fill(METRIC), plain_fill, "the plain fill after the refusals")
        again = ctx.fill_affinity(METRIC, group, n_groups, want_table=True)
        for key in AFFINITY_KEYS:
            same(again[key], plain_affinity[key], ("the plain affinity fill after the refusals", key))
        for arr, want in zip(again["table"], plain_affinity["table"]):
            same(arr, want, "the plain affinity table after the refusals")
        for arr, want in zip(multi.fill_between(METRIC, group, n_groups), plain_multi):
            same(arr, want, "the plain between fill on three devices after the refusals")
        # the clean triangle is taken, and so is one with -0.0 in place of zeros: a valid zero
        zeros = clean.copy()
        zeros[[0, 1, cases.pair_index(0, odd_row), cases.pair_index(30, 100), pairs - 1]] = -0.0
        zeros[[2, cases.pair_index(1, odd_row)]] = 0.0
        check_tree(ctx, zeros, n, "-0.0", slabs=(0, THREE_SLABS))
        hip.set_slab_values(zeros)
        check_between(ctx.fill_between, zeros, n, group, n_groups, "-0.0", slabs=(0, THREE_SLABS))
        check_affinity(ctx.fill_affinity, zeros, n, group, n_groups, "-0.0", slabs=(0, THREE_SLABS))
        check_between(multi.fill_between, zeros, n, group, n_groups, "-0.0 on three devices")
        # values of another collection's size: every slab fill refuses with PC_ERR_ARG
        hip.set_slab_values(cases.spread(n - 1, 102))
        for owner in (ctx, multi):
            for call in (lambda c: c.fill_edges(METRIC, 0.5), lambda c: c.fill_components(METRIC, 0.5), lambda c: c.fill_nearest(METRIC, 3),
                         lambda c: c.fill_tree(METRIC), lambda c: c.fill_between(METRIC, group, n_groups), lambda c: c.fill_affinity(METRIC, group, n_groups)):
                try:
                    call(owner)
                except hip.HipLibraryError as exc:
                    truth("status -1" in str(exc) and (owner is multi or f"{cases.n_pairs(n - 1)} values" in str(exc)), str(exc))
                else:
                    raise AssertionError("a triangle of the wrong size was taken")
        hip.set_slab_values(None)
        same(ctx.fill(METRIC), plain_fill, "the plain fill at the end")
        truth(ctx.shard_pairs() == pairs, "the unsharded context at the end")


CASES = {
    "tree": case_tree, "tree_tiny": case_tree_tiny,
    "components_edges_130": lambda: case_components_edges(130), "components_edges_515": lambda: case_components_edges(515),
    "components_edges_finite": case_components_edges_finite, "nearest": case_nearest,
    "between": case_between, "between_segment": case_between_segment,
    "affinity": case_affinity, "affinity_mean_tie": case_affinity_mean_tie, "affinity_ranges": case_affinity_ranges,
    "multi": case_multi, "refusals": case_refusals,
}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: slab_values_driver.py <" + " | ".join(CASES) + ">")
        return 2
    assert os.environ.get("PHAMCLUST_NATIVE_VARIANT") == "hooks" and hip.load().pc_test_hooks() == 1, "not the test-hooks twin of the library"
    CASES[argv[1]]()
    assert hip._slab_values is None, "a case left the hook set"
    print(f"ok {argv[1]} {COMPARED[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
