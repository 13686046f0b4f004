"""The child process of tests/test_gpu_rows_values.py: ``python rows_values_driver.py <case>`` under PHAMCLUST_NATIVE_VARIANT=hooks and
PHAMCLUST_NO_TORCH=1 (the variant is chosen when phamclust_amd.hip is imported, so the cases cannot run inside pytest's process).

Every case uploads ``hand_built(n)`` -- n genomes that share no pham; the collection only sets N --, injects a rows slab of
tests/rows_value_cases.py through ``hip.set_rows_values`` and compares what a rows form (``fill_rows_edges`` / ``_components`` /
``_tree`` / ``_nearest``) makes of it and of a contract-only seed with the plain reference there, exactly: ``np.array_equal`` on integers
or on the uint64 view of values.  Every slab is poisoned: its diagonal and, for the flat passes, the dead copy of every pair of two query
genomes hold a value that would change the result if a kernel read it.  Every input is also run once with the hook cleared, and the
expected result must differ from that: no comparison is vacuous.  A case asserts everything itself and ends with
``ok <case> <number of comparisons>``."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import rows_value_cases as rc                                                # noqa: E402
import slab_value_cases as tri                                               # noqa: E402
from phamclust_amd import hip                                                # noqa: E402
from slab_values_driver import COMPARED, METRIC, context, same, truth        # noqa: E402


def differs(got, want):
    """Some array of ``got`` is not ``want``'s, by shape or by bits."""
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return True
        if a.dtype == np.float64:
            a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)
        if not np.array_equal(a, b):
            return True
    return False


def slab_settings(m, n):
    """{slab_bytes: the slabs the walk must take}: all rows in one slab, the rows cut into at least three slabs where there are three
    rows, and one row per slab."""
    settings = {0: 1}
    for per in (max(m // 3, 1), 1):
        if m > 1:
            settings[8 * n * per + 7] = (m + per - 1) // per                 # (7 bytes that buy no row)
    return settings


def rows_arg(x):
    return x.rows.astype(np.int32)


# ---- the flat passes ---------------------------------------------------------------------------------------------------------
def check_flat(ctx, x, with_tree=True, must_differ=True):
    """The edge fill and both components fills at every threshold of the input, and the tree fill, under every slab setting.  Returns
    whether the expected results differ from what the calls return with the hook cleared."""
    n, rows, direction = x.n, rows_arg(x), dict(as_distance=x.as_distance)
    settings = slab_settings(rows.shape[0], n)
    truth(rows.shape[0] < 3 or max(settings.values()) >= 3, (x.label, "at least three slabs"))
    want_edges = {th: rc.edges(x.rows, x.slab, n, th, x.as_distance) for th in x.thresholds}
    want_labels = {(th, strict): rc.components(x.labels, x.rows, x.slab, n, th, x.as_distance, strict) for th in x.thresholds for strict in (True, False)}
    hip.set_rows_values(x.slab)
    for slab_bytes, slabs in settings.items():
        for th in x.thresholds:
            label = (x.label, float(th).hex(), slab_bytes)
            src, tgt, val, st = ctx.fill_rows_edges(METRIC, th, rows, slab_bytes=slab_bytes, want_stats=True, **direction)
            for got, stated, what in zip((src, tgt, val), want_edges[th], ("src", "tgt", "val")):
                same(got, stated, label + ("edges", what))
            truth(st["n_slabs"] == slabs and st["n_edges"] == want_edges[th][0].shape[0], label + ("edges", st["n_slabs"], slabs))
            for strict in (True, False):
                labels, cst = ctx.fill_rows_components(METRIC, th, rows, seed_labels=x.labels, strict=strict, slab_bytes=slab_bytes, want_stats=True, **direction)
                stated, n_pass = want_labels[th, strict]
                same(labels, stated, label + ("labels", strict))
                truth(cst["n_edges"] == n_pass and cst["n_components"] == np.unique(stated).shape[0] and cst["n_slabs"] == slabs,
                      label + ("counts", strict, cst["n_edges"], n_pass))
                if not strict:
                    truth(cst["n_edges"] == st["n_edges"], label + ("the non-strict count is the edge fill's",))
    want_tree = None
    if with_tree and x.tree_slab is not None:
        want_tree = rc.tree(x.forest, x.rows, x.tree_slab, n, x.as_distance)
        hip.set_rows_values(x.tree_slab)
        for slab_bytes, slabs in settings.items():
            src, tgt, val, st = ctx.fill_rows_tree(METRIC, rows, seed=x.forest, slab_bytes=slab_bytes, want_stats=True, **direction)
            for got, stated, what in zip((src, tgt, val), want_tree, ("src", "tgt", "val")):
                same(got, stated, (x.label, slab_bytes, "tree", what))
            truth(st["n_slabs"] == slabs and st["n_edges"] == n - 1, (x.label, slab_bytes, "tree", st["n_slabs"], slabs))
    # the hook cleared: the collection's own values, and none of what was expected above
    hip.set_rows_values(None)
    th = x.thresholds[-1]
    plain = ctx.fill_rows_edges(METRIC, th, rows, **direction)
    apart = differs(plain, want_edges[th])
    if want_tree is not None:
        apart = apart and differs(ctx.fill_rows_tree(METRIC, rows, seed=x.forest, **direction), want_tree)
    if must_differ:
        truth(apart, (x.label, "the expected results are not the unhooked call's"))
    return apart


def case_flat(n):
    with context(n) as ctx:
        for x in rc.flat_inputs(n):
            check_flat(ctx, x)


def case_flat_tiny():
    """n = 2 and 3 (where an expected result can be the collection's own: three values, one of them 1.0)."""
    for n in (2, 3):
        with context(n) as ctx:
            apart = [bool(check_flat(ctx, x, must_differ=False)) for x in rc.tiny_inputs() if x.n == n]
        truth(3 * sum(apart) >= len(apart) > 0, (n, "at least a third of the expected results are not the unhooked calls'", sum(apart), len(apart)))


def case_flat_wide():
    n, rows = rc.WIDE_SHAPE
    truth(len(rows) * n >= 3 * rc.CHUNK and n > rc.CHUNK, "a chunk inside one row, three chunks")
    with context(n) as ctx:
        for x in rc.wide_inputs():
            check_flat(ctx, x, with_tree=False)


# ---- nearest -----------------------------------------------------------------------------------------------------------------
def check_nearest(ctx, x, must_differ=True):
    n, rows, m = x.n, rows_arg(x), x.rows.shape[0]
    kk = min(x.k, n - 1)
    want = rc.nearest(x.seed, x.rows, x.slab, n, x.k, x.as_distance)
    settings = {0: 1}
    if m > 1:
        per = max(m // 3, 1)
        settings[8 * n * per] = (m + per - 1) // per
    hip.set_rows_values(x.slab)
    for slab_bytes, slabs in settings.items():
        nbr, val, st = ctx.fill_rows_nearest(METRIC, x.k, rows, seed=x.seed, as_distance=x.as_distance, slab_bytes=slab_bytes, want_stats=True)
        truth(st["k"] == kk and st["n_slabs"] == slabs, (x.label, slab_bytes, st["k"], st["n_slabs"], slabs))
        same(nbr, want[0], (x.label, slab_bytes, "nbr"))
        same(np.ascontiguousarray(val).view(np.uint64), want[1], (x.label, slab_bytes, "val"))
    hip.set_rows_values(None)
    plain = ctx.fill_rows_nearest(METRIC, x.k, rows, seed=x.seed, as_distance=x.as_distance)
    apart = differs((plain[0], np.ascontiguousarray(plain[1]).view(np.uint64)), want)
    if must_differ:
        truth(apart, (x.label, "the expected lists are not the unhooked call's"))
    return apart


def case_nearest(*shapes):
    """(At n = 2 and 3 an expected list can be the collection's own -- a tie_set value is the value of genomes that share no pham --,
    so there at least half of the inputs must differ from the unhooked call, not each.)"""
    for n in shapes:
        with context(n) as ctx:
            apart = [bool(check_nearest(ctx, x, must_differ=n > 3)) for x in rc.nearest_inputs(n)]
            truth(2 * sum(apart) >= len(apart), (n, "expected lists that are not the unhooked calls'", sum(apart), len(apart)))


# ---- the grow invariant under ties ---------------------------------------------------------------------------------------------
def case_grow():
    """N = 130: the seed is the triangular reference's result on the old block, and the rows form must deliver the triangular
    reference's result on the whole triangle -- what growing a stored result means, stated on values that tie."""
    n, k = 130, 64
    rows = rc.as_rows(sorted(set(range(3, n, 5)) | {0, 64, 65, n - 1}))
    rows32 = rows.astype(np.int32)
    with context(n) as ctx:
        for name, values in (("tie_set", tri.tie_set(n, 801)), ("two_valued", tri.rescaled(tri.two_valued(n, 0.5, 802), 499999, 500000))):
            old, old_values = rc.old_block(values, n, rows)
            n_old = old.shape[0]
            base = rc.rows_of(values, n, rows)
            for as_distance in (True, False):
                direction, best = dict(as_distance=as_distance), rc.best_value(as_distance)
                marked = rc.poisoned(base, rows, n, best, best)
                for slab_bytes in (0, 8 * n * 9):
                    label = ("grow", name, as_distance, slab_bytes)
                    hip.set_rows_values(marked)
                    for threshold in (0.5, 0.499999, 0.4999995, 0.0, 1.0):
                        got = ctx.fill_rows_edges(METRIC, threshold, rows32, slab_bytes=slab_bytes, **direction)
                        merged = rc.merged_edges(tri.edge_list(old_values, n_old, threshold, as_distance), old, got)
                        for arr, stated in zip(merged, tri.edge_list(values, n, threshold, as_distance)):
                            same(arr, stated, label + ("edges", threshold))
                        for strict in (True, False):
                            stored, stored_pass = tri.components(old_values, n_old, threshold, as_distance, strict)
                            seed = np.arange(n, dtype=np.int32)
                            seed[old] = old[stored]
                            labels, st = ctx.fill_rows_components(METRIC, threshold, rows32, seed_labels=seed, strict=strict, slab_bytes=slab_bytes,
                                                                  want_stats=True, **direction)
                            stated, whole_pass = tri.components(values, n, threshold, as_distance, strict)
                            same(labels, stated, label + ("labels", threshold, strict))
                            truth(st["n_edges"] == whole_pass - stored_pass, label + ("count", threshold, strict, st["n_edges"]))
                    nbr_old, val_old = tri.nearest(old_values, n_old, k, as_distance)
                    seed_nbr, seed_val = np.full((n, k), -7, dtype=np.int32), np.full((n, k), np.nan)
                    seed_nbr[old], seed_val[old] = old[nbr_old], val_old.view(np.float64)
                    hip.set_rows_values(rc.poisoned(base, rows, n, best))
                    nbr, val = ctx.fill_rows_nearest(METRIC, k, rows32, seed=(seed_nbr, seed_val), slab_bytes=slab_bytes, **direction)
                    stated = tri.nearest(values, n, k, as_distance)
                    same(nbr, stated[0], label + ("nbr",))
                    same(np.ascontiguousarray(val).view(np.uint64), stated[1], label + ("val",))
                    stored = tri.kruskal(old_values, n_old, as_distance)
                    hip.set_rows_values(rc.poisoned(base, rows, n, rc.NAN, rc.NAN))
                    got = ctx.fill_rows_tree(METRIC, rows32, seed=(old[stored[0]], old[stored[1]], stored[2]), slab_bytes=slab_bytes, **direction)
                    for arr, stated in zip(got, tri.kruskal(values, n, as_distance)):
                        same(arr, stated, label + ("tree",))
                hip.set_rows_values(None)
                truth(differs(ctx.fill_rows_tree(METRIC, rows32, seed=(old[stored[0]], old[stored[1]], stored[2]), **direction), tri.kruskal(values, n, as_distance)),
                      ("grow", name, as_distance, "the expected tree is not the unhooked call's"))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def refused(call, status, *texts):
    try:
        call()
    except hip.HipLibraryError as exc:
        truth(f"status {status}" in str(exc) and all(text in str(exc) for text in texts), str(exc))
    else:
        raise AssertionError(f"not refused with status {status}")


def case_refusals():
    n = 130
    rows = rc.as_rows([0, 1, 40, 63, 64, 65, 100, 128, 129])
    rows32, m = rows.astype(np.int32), 9
    values = tri.spread(n, 901)
    base = rc.rows_of(values, n, rows)
    clean = rc.poisoned(base, rows, n, rc.NAN, rc.NAN)
    forest, labels = rc.forest_seed(n, rows, 902), rc.labelling_seed(n, rows, 903)
    lists = rc.lists_seed(n, rows, 5, 904, pool=tri.of_micros(tri.TIE_MICROS))
    live = np.argwhere(rc.live_mask(rows, n))
    dead = np.argwhere(~rc.live_mask(rows, n))
    # live places of every kind: the first and the last live element, an odd element at a row's end, a row's first, a pair of two query genomes
    places = [tuple(live[0]), tuple(live[-1]), (0, n - 1), (2, 2), (3, 2), (2, 63), (5, 129), (4, 66)]
    truth(all(rc.live_mask(rows, n)[p] for p in places) and rc.query_mask(rows, n)[63] and (0 * n + n - 1) % 2 == 1, "the places are live")
    calls = {"edges": lambda c, **kw: c.fill_rows_edges(METRIC, 0.5, rows32, **kw), "components": lambda c, **kw: c.fill_rows_components(METRIC, 0.5, rows32, seed_labels=labels, **kw),
             "tree": lambda c, **kw: c.fill_rows_tree(METRIC, rows32, seed=forest, **kw), "nearest": lambda c, **kw: c.fill_rows_nearest(METRIC, 5, rows32, seed=lists, **kw)}
    with context(n) as ctx:
        plain = {name: call(ctx) for name, call in calls.items()}
        plain_triangular = ctx.fill_edges(METRIC, 0.5)
        want = rc.tree(forest, rows, clean, n)
        truth(differs(plain["tree"], want), "the expected tree is not the unhooked call's")
        # a live element that is no millionth in [0, 1]: PC_ERR_DATA, wherever it lies and however the rows are cut
        for i, bad in enumerate(tri.BAD_VALUES):
            for place in (places[i % len(places)], places[(i + 3) % len(places)], places[(2 * i + 1) % len(places)]):
                marked = clean.copy()
                marked[place] = bad
                hip.set_rows_values(marked)
                for slab_bytes in (0, 8 * n * 3, 8 * n):
                    refused(lambda: ctx.fill_rows_tree(METRIC, rows32, seed=forest, slab_bytes=slab_bytes), -5, "pc_fill_rows_tree", "no millionth in [0, 1]")
        # the same values in every dead element: never read, the tree is the reference's
        for bad in tri.BAD_VALUES:
            marked = rc.poisoned(base, rows, n, bad, bad)
            truth(bool((~rc.live_mask(rows, n)).sum() == m + m * (m - 1) // 2 == dead.shape[0]), "the dead elements")
            hip.set_rows_values(marked)
            for slab_bytes in (0, 8 * n * 3, 8 * n):
                for got, stated in zip(ctx.fill_rows_tree(METRIC, rows32, seed=forest, slab_bytes=slab_bytes), want):
                    same(got, stated, ("dead elements hold", bad, slab_bytes))
        # a hook of another size: PC_ERR_ARG from every rows form, nothing else disturbed
        for wrong in (np.zeros((m - 1, n)), np.zeros((m + 1, n)), np.zeros((m, n - 1)), np.zeros((n, m))):
            hip.set_rows_values(wrong)
            for name, call in calls.items():
                refused(lambda: call(ctx), -1, "pc_hook_rows_values", f"{wrong.shape[0]} rows of {wrong.shape[1]} values")
            for got, stated in zip(ctx.fill_edges(METRIC, 0.5), plain_triangular):
                same(got, stated, "the triangular walk does not read the rows hook")
        # the hook cleared: the collection's own results again
        hip.set_rows_values(None)
        for name, call in calls.items():
            for got, stated in zip(call(ctx) if name != "components" else (call(ctx),), plain[name] if name != "components" else (plain[name],)):
                same(got, stated, ("the plain result after the refusals", name))
        # only the triangular hook set: the rows forms are the collection's; only the rows hook set: the triangular fills are
        hip.set_slab_values(values)
        truth(differs(ctx.fill_edges(METRIC, 0.5), plain_triangular), "the triangular hook is in force")
        for name, call in calls.items():
            for got, stated in zip(call(ctx) if name != "components" else (call(ctx),), plain[name] if name != "components" else (plain[name],)):
                same(got, stated, ("the rows form under the triangular hook", name))
        hip.set_rows_values(rc.poisoned(base, rows, n, 0.0, 0.0))
        for got, stated in zip(ctx.fill_edges(METRIC, 0.5), tri.edge_list(values, n, 0.5)):
            same(got, stated, "the triangular fill under both hooks is the triangle's")
        truth(differs(calls["edges"](ctx), plain["edges"]), "the rows hook is in force beside the triangular one")
        hip.set_slab_values(None)
        for got, stated in zip(ctx.fill_edges(METRIC, 0.5), plain_triangular):
            same(got, stated, "the triangular fill under the rows hook alone")
        for arr, stated in zip(ctx.fill_tree(METRIC), ctx.fill_tree(METRIC, slab_bytes=8 * 1000)):
            same(arr, stated, "the triangular tree under the rows hook alone")
        hip.set_rows_values(None)


CASES = {
    "flat_tiny": case_flat_tiny, "flat_63": lambda: case_flat(63), "flat_64": lambda: case_flat(64), "flat_65": lambda: case_flat(65),
    "flat_511": lambda: case_flat(511), "flat_512": lambda: case_flat(512), "flat_513": lambda: case_flat(513), "flat_wide": case_flat_wide,
    "grow": case_grow, "nearest_tiny": lambda: case_nearest(2, 3), "nearest_64": lambda: case_nearest(64), "nearest_65": lambda: case_nearest(65),
    "nearest_129": lambda: case_nearest(129), "nearest_130": lambda: case_nearest(130), "refusals": case_refusals,
}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: rows_values_driver.py <" + " | ".join(CASES) + ">")
        return 2
    assert os.environ.get("PHAMCLUST_NATIVE_VARIANT") == "hooks" and hip.load().pc_test_hooks() == 1, "not the test-hooks twin of the library"
    CASES[argv[1]]()
    assert hip._rows_values is None and hip._slab_values is None, "a case left a hook set"
    print(f"ok {argv[1]} {COMPARED[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
