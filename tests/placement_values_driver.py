"""The child process of tests/test_gpu_placement_values.py: ``python placement_values_driver.py <case>`` under
PHAMCLUST_NATIVE_VARIANT=hooks and PHAMCLUST_NO_TORCH=1 (the variant is chosen when phamclust_amd.hip is imported, so the cases cannot run
inside pytest's process).

Every case uploads ``hand_built(n)`` -- n genomes that share no pham; the collection only sets N --, injects a rows slab of
tests/placement_value_cases.py through ``hip.set_rows_values`` and compares what ``fill_rows_affinity`` makes of it with
``GroupPlacement.from_dense`` of the input's matrix, exactly (``np.array_equal`` on integers), in both directions, in one slab and one
row per slab.  Every slab is poisoned: its diagonal and the columns of unlabelled genomes hold NaN, which would fail the call if a
kernel read it.  Every shape is also run once with the hook cleared, and the expected result must differ from that: no comparison is
vacuous.  A case asserts everything itself and ends with ``ok <case> <number of comparisons>``."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import placement_value_cases as pv                                           # noqa: E402
from phamclust_amd import hip                                                # noqa: E402
from slab_values_driver import COMPARED, METRIC, context, same, truth        # noqa: E402

ARRAYS = ("own_sum", "own_lo", "own_hi", "near_group", "near_sum", "near_lo", "near_hi")


def compare(got, want, label):
    for name in ARRAYS:
        same(got[name], getattr(want, name), label + (name,))
    for part in ("table", "gain"):
        for arr, stated in zip(got[part], getattr(want, part)):
            same(arr, stated, label + (part,))


def differs(got, want):
    return any(not np.array_equal(got[name], getattr(want, name)) for name in ARRAYS)


def check(ctx, x):
    want = x.expected()
    wants = {True: want, False: want.inverted()}
    m = x.rows.shape[0]
    hip.set_rows_values(x.slab())
    for slab_bytes, slabs in ((0, 1), (8 * x.n + 7, m)):
        for as_distance in (True, False):
            got = ctx.fill_rows_affinity(METRIC, x.label, x.rows, x.n_groups, as_distance=as_distance, slab_bytes=slab_bytes, want_table=True, want_gain=True,
                                         want_stats=True)
            truth(got["stats"]["n_slabs"] == slabs, (x.tag, slab_bytes, got["stats"]["n_slabs"], slabs))
            compare(got, wants[as_distance], (x.tag, slab_bytes, as_distance))
    hip.set_rows_values(None)
    return want


def case_shape(n):
    with context(n) as ctx:
        apart = []
        for x in pv.inputs(n):
            want = check(ctx, x)
            plain = ctx.fill_rows_affinity(METRIC, x.label, x.rows, x.n_groups)
            apart.append(differs(plain, want))
        # (genomes that share no pham are all at distance 1: a constant slab of another value, or a labelling with no second group,
        # can state the same nearest groups and values only where there is nothing to state)
        truth(2 * sum(apart) >= len(apart), (n, "expected results that are not the unhooked calls'", sum(apart), len(apart)))


def case_wide():
    """One entry takes 4,299 values of 10^6: above 2^32."""
    x = pv.wide_input()
    with context(x.n) as ctx:
        want = check(ctx, x)
        truth(int(want.own_sum[0]) == (pv.WIDE - 1) * pv.MILLION > 2**32 and int(want.gain[0][1]) == 2 * pv.MILLION, "the sums")


def refused(call, status, *texts):
    try:
        call()
    except hip.HipLibraryError as exc:
        truth(f"status {status}" in str(exc) and all(text in str(exc) for text in texts), str(exc))
    else:
        raise AssertionError(f"not refused with status {status}")


def case_refusals():
    """A refused value (NaN, 1 + ulp, no millionth) where a pass reads it: PC_ERR_DATA with the number of PAIRS, under both slab cuts; a
    clean call follows on the same context."""
    cases = pv.refused_inputs()
    x = cases[0][1]
    want = x.expected()
    with context(x.n) as ctx:
        for tag, _, slab, pairs in cases:
            hip.set_rows_values(slab)
            for slab_bytes in (0, 8 * x.n * 2, 8 * x.n):
                for want_gain in (False, True):
                    refused(lambda: ctx.fill_rows_affinity(METRIC, x.label, x.rows, x.n_groups, slab_bytes=slab_bytes, want_gain=want_gain), -5,
                            "pc_fill_rows_affinity", f": {pairs} pairs of the call", "no millionth in [0, 1]")
            hip.set_rows_values(x.slab())
            got = ctx.fill_rows_affinity(METRIC, x.label, x.rows, x.n_groups, want_table=True, want_gain=True)
            compare(got, want, (tag, "the clean call after the refusal"))
        # a hook of another size: PC_ERR_ARG, nothing else disturbed
        for wrong in (np.zeros((len(x.rows) - 1, x.n)), np.zeros((len(x.rows), x.n + 1))):
            hip.set_rows_values(wrong)
            refused(lambda: ctx.fill_rows_affinity(METRIC, x.label, x.rows, x.n_groups), -1, "pc_hook_rows_values")
        hip.set_rows_values(None)
        plain = ctx.fill_rows_affinity(METRIC, x.label, x.rows, x.n_groups, want_table=True)
        whole = ctx.fill_affinity(METRIC, np.maximum(x.label, 0), x.n_groups, want_table=True)
        truth(differs(plain, want), "the expected result is not the unhooked call's")
        same(plain["table"][0][:, 1:], whole["table"][0][x.rows][:, 1:], "the unhooked call is the collection's")


CASES = {
    "tiny": lambda: [case_shape(n) for n in (2, 3)], "n63": lambda: case_shape(63), "n64": lambda: case_shape(64), "n65": lambda: case_shape(65),
    "n255": lambda: case_shape(255), "n256": lambda: case_shape(256), "n257": lambda: case_shape(257), "n513": lambda: case_shape(513),
    "wide": case_wide, "refusals": case_refusals,
}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: placement_values_driver.py <" + " | ".join(CASES) + ">")
        return 2
    assert os.environ.get("PHAMCLUST_NATIVE_VARIANT") == "hooks" and hip.load().pc_test_hooks() == 1, "not the test-hooks twin of the library"
    CASES[argv[1]]()
    assert hip._rows_values is None and hip._slab_values is None, "a case left a hook set"
    print(f"ok {argv[1]} {COMPARED[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
