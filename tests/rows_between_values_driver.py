"""The child process of tests/test_gpu_rows_between_values.py: ``python rows_between_values_driver.py <case>`` under
PHAMCLUST_NATIVE_VARIANT=hooks and PHAMCLUST_NO_TORCH=1 (the variant is chosen when phamclust_amd.hip is imported, so the cases cannot run
inside pytest's process).

Every case uploads ``hand_built(n)`` -- n genomes that share no pham; the collection only sets N --, injects a rows slab of
tests/rows_between_value_cases.py through ``hip.set_rows_values`` and compares what ``fill_rows_between`` makes of it with the plain loops
of that file, exactly (``np.array_equal`` on integers): in both directions, in one slab and one row per slab, without a seed and with a
seed that satisfies nothing but the contract.  Every slab is poisoned where no pass may read (0.5, which no live element holds, and 2.0,
which would fail the call).  A case asserts everything itself and ends with ``ok <case> <number of comparisons>``."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import rows_between_value_cases as bv                                        # noqa: E402
from phamclust_amd import hip                                                # noqa: E402
from slab_values_driver import COMPARED, METRIC, context, same, truth        # noqa: E402

NAMES = ("sum", "count", "lo", "hi")


def compare(got, want, label):
    for arr, stated, name in zip(got, want, NAMES):
        same(arr, stated, label + (name,))


def check(ctx, x, cuts=None, seeded=True):
    m = x.rows.shape[0]
    hip.set_rows_values(x.slab())
    for as_distance in (True, False):
        table = x.table(as_distance)
        truth(np.array_equal(table[1], table[1].T), (x.tag, "the reference is symmetric"))
        for slab_bytes, slabs in cuts or ((0, 1), (8 * x.n + 7, m)):
            *got, st = ctx.fill_rows_between(METRIC, x.label, x.rows, x.n_groups, as_distance=as_distance, slab_bytes=slab_bytes, want_stats=True)
            truth(st["n_slabs"] == slabs, (x.tag, slab_bytes, st["n_slabs"], slabs))
            compare(got, table, (x.tag, "no seed", as_distance, slab_bytes))
            if seeded:
                seed = x.contract_seed(len(x.tag) + int(as_distance))
                got = ctx.fill_rows_between(METRIC, x.label, x.rows, x.n_groups, seed=seed, as_distance=as_distance, slab_bytes=slab_bytes)
                compare(got, bv.combined(seed, table), (x.tag, "seed", as_distance, slab_bytes))
    hip.set_rows_values(None)


def case_shapes(*shapes, all_rows=False):
    truth(hip.Context.between_segment() == bv.SEGMENT, "PC_BETWEEN_SEGMENT")
    for n in shapes:
        with context(n) as ctx:
            apart = 0
            inputs = bv.inputs(n, all_rows=all_rows)
            for x in inputs:
                check(ctx, x)
                # (genomes that share no pham are all at distance 1: the unhooked call states another table wherever there is a pair)
                plain = ctx.fill_rows_between(METRIC, x.label, x.rows, x.n_groups)
                apart += not np.array_equal(plain[0], x.table()[0])
            truth(n <= 3 or 2 * apart >= len(inputs), (n, "expected tables that are not the unhooked calls'", apart, len(inputs)))


def case_many_groups():
    x = bv.many_groups_input()
    with context(x.n) as ctx:
        check(ctx, x, cuts=((0, 1), (8 * x.n, 3)))


def refused(call, status, *texts):
    try:
        call()
    except hip.HipLibraryError as exc:
        truth(f"status {status}" in str(exc) and all(text in str(exc) for text in texts), str(exc))
    else:
        raise AssertionError(f"not refused with status {status}")


def case_refusals():
    """A live 2.0 and a live 0.1234565: PC_ERR_DATA with the number of refused values, each pair once, under both slab cuts and with a
    seed; a clean call follows on the same context."""
    cases = bv.refused_inputs()
    x = cases[0][1]
    want = x.table()
    seed = x.contract_seed(5)
    with context(x.n) as ctx:
        for tag, _, slab, pairs in cases:
            hip.set_rows_values(slab)
            for slab_bytes in (0, 8 * x.n):
                for given in (None, seed):
                    refused(lambda: ctx.fill_rows_between(METRIC, x.label, x.rows, x.n_groups, seed=given, slab_bytes=slab_bytes), -5,
                            "pc_fill_rows_between", f": {pairs} values of the fill", "no millionth in [0, 1]")
            hip.set_rows_values(x.slab())
            compare(ctx.fill_rows_between(METRIC, x.label, x.rows, x.n_groups), want, (tag, "the clean call after the refusal"))
        hip.set_rows_values(None)


CASES = {
    "tiny": lambda: case_shapes(2, 3), "n63": lambda: case_shapes(63), "n64": lambda: case_shapes(64), "n65": lambda: case_shapes(65),
    "n65_all": lambda: case_shapes(65, all_rows=True), "n4095": lambda: case_shapes(4095), "n4096": lambda: case_shapes(4096),
    "n4097": lambda: case_shapes(4097), "n8193": lambda: case_shapes(8193), "many_groups": case_many_groups, "refusals": case_refusals,
}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: rows_between_values_driver.py <" + " | ".join(CASES) + ">")
        return 2
    assert os.environ.get("PHAMCLUST_NATIVE_VARIANT") == "hooks" and hip.load().pc_test_hooks() == 1, "not the test-hooks twin of the library"
    CASES[argv[1]]()
    assert hip._rows_values is None and hip._slab_values is None, "a case left a hook set"
    print(f"ok {argv[1]} {COMPARED[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
