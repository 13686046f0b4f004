"""The child process of tests/test_gpu_hist_values.py: ``python hist_values_driver.py <case>`` under PHAMCLUST_NATIVE_VARIANT=hooks and
PHAMCLUST_NO_TORCH=1 (the variant is chosen when phamclust_amd.hip is imported, so the cases cannot run inside pytest's process).

Every case uploads ``hand_built(n)`` -- the collection only sets N --, injects a value triangle through ``hip.set_slab_values`` (the rows
case: a rows slab through ``hip.set_rows_values``) and compares what the distribution fill makes of it with the reference of
tests/hist_value_cases.py, integer for integer.  It asserts everything itself and ends with ``ok <case> <number of comparisons>``."""

import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import hist_value_cases as cases                                            # noqa: E402
import rows_value_cases as rowcases                                         # noqa: E402
import slab_value_cases as tri                                              # noqa: E402
from phamclust_amd import hip                                                # noqa: E402

METRIC = "jc"
MILLION = cases.MILLION
COMPARED = [0]


def same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        first = np.argwhere(got != want)[0].tolist()
        raise AssertionError(f"{label}: {int((got != want).sum())} of {got.size} bins differ, the first at {first}: "
                             f"{got[tuple(first)]!r} for {want[tuple(first)]!r}")
    COMPARED[0] += 1


def truth(condition, label):
    assert condition, label
    COMPARED[0] += 1


def hand_built(n):
    """n genomes of four genes each that share no pham."""
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


def check(fill_hist, values, n, label, group=None, n_groups=None, slabs=(0,), directions=(True, False)):
    """The fill on an injected triangle, every cut and both directions, against the reference."""
    hip.set_slab_values(values)
    for as_distance in directions:
        want = cases.hist(values, n, group, as_distance)
        for slab_bytes in slabs:
            got, st = fill_hist(METRIC, group, n_groups, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
            same(got, want, (label, as_distance, slab_bytes))
            truth(st["hist_pairs"] == tri.n_pairs(n) and st["n_classes"] == want.shape[0], (label, "counts", st["hist_pairs"], st["n_classes"]))
            if "per_device" not in st:
                truth(st["n_slabs"] == n_slabs(n, slab_bytes), (label, "slabs", slab_bytes, st["n_slabs"]))
    hip.set_slab_values(None)


def case_hot():
    n = 130
    pairs = tri.n_pairs(n)
    assert pairs == 8385 and pairs > 2 * cases.CHUNK
    with context(n) as ctx:
        for value, bin_at in ((1.0, MILLION), (0.0, 0), (-0.0, 0)):
            values = cases.constant(n, value)
            check(ctx.fill_hist, values, n, ("all", value))
            hip.set_slab_values(values)
            got = ctx.fill_hist(METRIC)
            hip.set_slab_values(None)
            truth(int(got[0, bin_at]) == pairs and int(got.sum()) == pairs, ("one bin holds every pair", value))
        check(ctx.fill_hist, cases.rotation(n, [0, MILLION]), n, "0 and 1 alternate")
        check(ctx.fill_hist, cases.rotation(n, [250000, 250001]), n, "two neighbours alternate")
        check(ctx.fill_hist, cases.rotation(n, np.arange(65) * 15000), n, "65 values in rotation")
        check(ctx.fill_hist, cases.rotation(n, [0, 0, 0, 7, MILLION, MILLION]), n, "three hot values", slabs=(0, 8 * 3000))


def case_distinct():
    n = 130
    assert cases.CHUNK > hip.Context.hist_table_slots(), "a chunk of distinct values must overflow the table"
    with context(n) as ctx:
        for descending in (False, True):
            values = cases.all_distinct(n, descending)
            assert np.unique(values).shape[0] == tri.n_pairs(n)
            check(ctx.fill_hist, values, n, ("distinct", descending), slabs=(0, 8 * 3000))
            hip.set_slab_values(values)
            got = ctx.fill_hist(METRIC)
            hip.set_slab_values(None)
            truth(int(got.max()) == 1 and int(got.sum()) == tri.n_pairs(n), ("every bin exactly 1", descending))
        group, n_groups = cases.labelings(n)["round-robin 5"]
        check(ctx.fill_hist, cases.all_distinct(n), n, "distinct, partitioned", group, n_groups)
        check(ctx.fill_hist, tri.ramp(n), n, "ramp", slabs=(0, 8 * 1000))


def case_collide():
    n = 130
    slots, probes = hip.Context.hist_table_slots(), hip.Context.hist_probes()
    micros = cases.colliding_micros(slots, probes + 12)
    truth(len({hip.Context.hist_slot(int(m)) for m in micros}) == 1 and cases.slot_of(int(micros[0]), slots) == hip.Context.hist_slot(int(micros[0])),
          "the keys share their first slot, by the documented hash")
    with context(n) as ctx:
        for seed in (31, 32):
            check(ctx.fill_hist, cases.collide(n, slots, probes, seed), n, ("collide", seed), slabs=(0, 8 * 3000))
        # the same run of keys, each element another of them in turn: every chunk meets all of them
        check(ctx.fill_hist, cases.rotation(n, np.concatenate([micros, [0, MILLION]])), n, "collide in rotation")


def case_seams():
    for n in (92, 91):
        assert tri.n_pairs(92) == cases.CHUNK + 90 and tri.n_pairs(91) % 2 == 1
        with context(n) as ctx:
            slabs = (0, 8 * 2200, 8 * 300, 8)
            assert [n_slabs(n, s) for s in slabs][:2] == [1, 2] and n_slabs(n, 8 * 300) > 8
            check(ctx.fill_hist, tri.spread(n, 40 + n), n, ("seams", n), slabs=slabs)
            group, n_groups = cases.labelings(n)["round-robin 5"]
            check(ctx.fill_hist, tri.tie_set(n, 50 + n), n, ("seams, partitioned", n), group, n_groups, slabs=slabs)
    for n in (2, 3):
        with context(n) as ctx:
            for micros in ([0] * tri.n_pairs(n), [MILLION] * tri.n_pairs(n), list(range(500000, 500000 + tri.n_pairs(n)))):
                check(ctx.fill_hist, tri.of_micros(micros), n, ("tiny", n, micros[0]), slabs=(0, 8))
                check(ctx.fill_hist, tri.of_micros(micros), n, ("tiny, partitioned", n, micros[0]), np.arange(n, dtype=np.int32) % 2, 2, slabs=(0, 8))


def case_partition():
    n = 130
    with context(n) as ctx:
        for name, (group, n_groups) in cases.labelings(n).items():
            for values, what in ((cases.by_class(n, group, 123456, 654321), "by class"), (cases.by_class(n, group, 0, 0), "one value"),
                                 (tri.tie_set(n, 61), "tie set"), (tri.spread(n, 62), "spread")):
                check(ctx.fill_hist, values, n, (name, what), group, n_groups, slabs=(0, 8 * 3000))
            hip.set_slab_values(tri.spread(n, 63))
            got = ctx.fill_hist(METRIC, group, n_groups)
            back = ctx.fill_hist(METRIC, group, n_groups, as_distance=False)
            hip.set_slab_values(None)
            truth(int(got[0].sum()) == cases.within_pairs(group) and int(got.sum()) == tri.n_pairs(n), (name, "class 0 totals the within pairs"))
            same(back, np.ascontiguousarray(got[:, ::-1]), (name, "the similarity form is the reversed bins"))
        # labels are only compared: no cap on their range
        check(ctx.fill_hist, tri.tie_set(n, 64), n, "sparse labels", (np.arange(n, dtype=np.int32) % 7) * 100000, 700000)


def expect_refusal(call, status, *needles):
    try:
        call()
    except hip.HipLibraryError as exc:
        truth(f"status {status}" in str(exc) and all(x in str(exc) for x in needles), str(exc))
        return str(exc)
    raise AssertionError(f"not refused: expected status {status} with {needles}")


def case_rows():
    n = 92
    triangle = tri.tie_set(n, 71)
    spread = tri.spread(n, 72)
    group, n_groups = cases.labelings(n)["round-robin 5"]
    poisons = ((7.0, float("nan")), (float("nan"), -1.0), (-1.0, 7.0))
    with context(n) as ctx:
        sets = rowcases.query_sets(n, with_all=True)
        sets["scattered"] = rowcases.as_rows([3, 17, 18, 40, 77, 91])
        for k, (name, rows) in enumerate(sorted(sets.items())):
            values = triangle if k % 2 == 0 else spread
            old = ~rowcases.query_mask(rows, n)
            diagonal, dead = poisons[k % 3]
            slab = rowcases.poisoned(rowcases.rows_of(values, n, rows), rows, n, diagonal, dead)
            hip.set_rows_values(slab)
            for part, parts in ((None, None), (group, n_groups)):
                for as_distance in (True, False):
                    whole = cases.hist(values, n, part, as_distance)
                    seed = cases.hist_among(values, n, old, part, as_distance)
                    for slab_bytes in (0, 8 * n * 2):
                        got, st = ctx.fill_rows_hist(METRIC, rows, group=part, n_groups=parts, seed=seed, as_distance=as_distance, slab_bytes=slab_bytes,
                                                     want_stats=True)
                        same(got, whole, (name, "seed + rows is the whole", part is not None, as_distance, slab_bytes))
                        truth(st["hist_pairs"] == tri.n_pairs(n) and st["n_slabs"] == hip.Context.rows_slabs(n, len(rows), slab_bytes or 8 * n * n),
                              (name, "counts", st["hist_pairs"], st["n_slabs"]))
                    alone = ctx.fill_rows_hist(METRIC, rows, group=part, n_groups=parts, as_distance=as_distance)
                    same(alone, whole - seed, (name, "no seed: the pairs with a query end alone", part is not None, as_distance))
            hip.set_rows_values(None)
        # the seed refusals
        rows = sets["adjacent"]
        old = ~rowcases.query_mask(rows, n)
        hip.set_rows_values(rowcases.rows_of(triangle, n, rows))
        seed = cases.hist_among(triangle, n, old, group)
        at = int(np.flatnonzero(seed[0])[0])
        negative = seed.copy(); negative[0, at] -= seed[0, at] + 1; negative[1, at] += seed[0, at] + 1
        expect_refusal(lambda: ctx.fill_rows_hist(METRIC, rows, group=group, n_groups=n_groups, seed=negative), -1, "pc_fill_rows_hist", "negative")
        short = seed.copy(); short[0, at] -= 1
        expect_refusal(lambda: ctx.fill_rows_hist(METRIC, rows, group=group, n_groups=n_groups, seed=short), -1, "pc_fill_rows_hist", "another genome set")
        moved = seed.copy(); moved[0, at] -= 1; moved[1, at] += 1
        expect_refusal(lambda: ctx.fill_rows_hist(METRIC, rows, group=group, n_groups=n_groups, seed=moved), -1, "pc_fill_rows_hist", "class 0")
        unlabelled = group.copy(); unlabelled[5] = -1
        expect_refusal(lambda: ctx.fill_rows_hist(METRIC, rows, group=unlabelled, n_groups=n_groups), -1, "genome 5 has label -1")
        same(ctx.fill_rows_hist(METRIC, rows, group=group, n_groups=n_groups, seed=seed), cases.hist(triangle, n, group), "after the refusals")
        # a refused value in a live element is counted once per pair; in a dead one it is not looked at
        bad = rowcases.rows_of(triangle, n, rows)
        bad[0, 0] = float("nan"); bad[1, 5] = 2.0
        hip.set_rows_values(bad)
        message = expect_refusal(lambda: ctx.fill_rows_hist(METRIC, rows), -5, "pc_fill_rows_hist")
        truth(counted(message) == 2, message)
        hip.set_rows_values(None)


def case_multi():
    n = 130
    packed = hand_built(n)
    group, n_groups = cases.labelings(n)["blocks of 32"]
    with hip.Context(0) as ctx:
        ctx.upload(packed, residues=False)
        for world in (2, 3):
            with hip.MultiContext([0] * world) as multi:
                multi.upload(packed, residues=False)
                for values, what in ((tri.spread(n, 81), "spread"), (cases.constant(n, 1.0), "all 1.0"), (cases.all_distinct(n), "distinct")):
                    check(multi.fill_hist, values, n, (world, what), slabs=(0, 8 * 1000))
                    check(multi.fill_hist, values, n, (world, what, "partitioned"), group, n_groups)
                    hip.set_slab_values(values)
                    same(multi.fill_hist(METRIC, group, n_groups), ctx.fill_hist(METRIC, group, n_groups), (world, what, "the single context's"))
                    hip.set_slab_values(None)


def counted(message):
    found = re.search(r": (\d+) values of the fill are no millionth in \[0, 1\]", message)
    assert found, message
    return int(found.group(1))


def case_refusals():
    n = 130
    pairs = tri.n_pairs(n)
    positions = [0, pairs - 1, tri.pair_index(0, 57), tri.pair_index(56, 57), tri.pair_index(0, 58), tri.pair_index(20, 40), tri.pair_index(50, 90),
                 tri.pair_index(100, 120), cases.CHUNK - 1, cases.CHUNK]
    assert len(set(positions)) == len(positions)
    clean = tri.spread(n, 91)
    group, n_groups = cases.labelings(n)["round-robin 5"]
    packed = hand_built(n)
    with hip.Context(0) as ctx, hip.MultiContext([0] * 3) as multi:
        ctx.upload(packed, residues=False)
        multi.upload(packed, residues=False)
        plain = ctx.fill_hist(METRIC, group, n_groups)
        same(plain.sum(axis=0), np.bincount(np.rint(ctx.fill(METRIC) * 1.0e6).astype(np.int64), minlength=cases.BINS), "the real fill's histogram")
        for k, value in enumerate(cases.BAD_VALUES):                          # each kind alone: exactly one value refused
            one = clean.copy()
            one[positions[k]] = value
            hip.set_slab_values(one)
            message = expect_refusal(lambda: ctx.fill_hist(METRIC), -5, "pc_fill_hist")
            truth(counted(message) == 1, (value, message))
        hip.set_slab_values(cases.with_bad(clean, positions))
        for owner, name in ((ctx, "pc_fill_hist"), (multi, "pc_multi_fill_hist")):
            for part, parts in ((None, None), (group, n_groups)):
                for slab_bytes in (0, 8 * 3000):
                    message = expect_refusal(lambda: owner.fill_hist(METRIC, part, parts, slab_bytes=slab_bytes), -5, name)
                    truth(counted(message) == len(positions), (name, slab_bytes, message))
        # a refused walk leaves the context whole: the next calls are correct
        hip.set_slab_values(None)
        same(ctx.fill_hist(METRIC, group, n_groups), plain, "the plain fill after the refusals")
        same(multi.fill_hist(METRIC, group, n_groups), plain, "the plain fill on three devices after the refusals")
        check(ctx.fill_hist, clean, n, "the clean triangle after the refusals", group, n_groups)
        zeros = clean.copy()
        zeros[[0, 1, tri.pair_index(30, 100), pairs - 1]] = -0.0
        check(ctx.fill_hist, zeros, n, "-0.0 is the millionth 0", slabs=(0, 8 * 3000))
        # the other refusals, in pc_fill_between's wording
        expect_refusal(lambda: ctx.fill_hist(METRIC, np.where(np.arange(n) == 3, 5, group).astype(np.int32), n_groups), -1, "genome 3 has label 5, outside [0, 5)")
        expect_refusal(lambda: ctx.fill_hist(METRIC, group, 0), -1, "n_groups 0")
        expect_refusal(lambda: ctx.fill_hist(METRIC, slab_bytes=-1), -1, "slab_bytes -1")
        same(ctx.fill_hist(METRIC, group, n_groups), plain, "the plain fill at the end")
    with context(1) as ctx:
        got, st = ctx.fill_hist(METRIC, want_stats=True)
        truth(got.shape == (1, cases.BINS) and not got.any() and st["hist_pairs"] == 0 and st["n_slabs"] == 0, "one genome: every bin zero")


CASES = {"hot": case_hot, "distinct": case_distinct, "collide": case_collide, "seams": case_seams, "partition": case_partition, "rows": case_rows,
         "multi": case_multi, "refusals": case_refusals}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: hist_values_driver.py <" + " | ".join(CASES) + ">")
        return 2
    assert os.environ.get("PHAMCLUST_NATIVE_VARIANT") == "hooks" and hip.load().pc_test_hooks() == 1, "not the test-hooks twin of the library"
    CASES[argv[1]]()
    assert hip._slab_values is None and hip._rows_values is None, "a case left a hook set"
    print(f"ok {argv[1]} {COMPARED[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
