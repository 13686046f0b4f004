"""The classes the rate table moved (run with ``-m gpu``).

* Every column length at which the table's variant differs from the model's (found on the CPU from the two, tests/chooser_table_cases.py),
  the length before and after each run of them, and the two lengths tests/test_host.py pins (100 and 650 residues) -- each with buckets of
  1, nseg, nseg + 1 and 40 rows and one "any byte" column gene, through pc_fill itself: peq, and aai with percent-positives, under tie rules
  0 and 3, the strip path as the launcher chooses and with PC_PIPE=0, whole matrices against the oracle bit for bit.
* Every launch class (W, lanes-per-segment bucket) whose CELL the table changed, whether or not a moved variant lands on it: one length in
  the bucket, forced onto that variant through pc_align_pairs, in the class's own workgroup and cut as a fill cuts it (two-wave tasks run
  the class's cell too), against the oracle's alignments.
* The switches this table brought (PC_RATE_TABLE, PC_CHOOSE_MAX_W, PC_INC16=2), each in a process of its own: the same matrices.

The smallest shapes at which a wrong class, cell or LDS size can show.
"""

import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import chooser_table_cases as ct
import planner_cases as pc

pytestmark = pytest.mark.gpu
KNOB_LENGTHS = (700, 1000)                          # W = 11 / W = 16 on 64 lanes: where PC_INC16=2 puts the profile cell on one segment per wave


def changed_cells(table):
    """[(W, bucket, length)] -- launch classes whose cell is not the model's, with a column length whose segments fall in the bucket"""
    out = []
    for W in ct.VARIANTS:
        for Gb in (8, 16, 32):
            if W <= ct.INC16_MAX_W and table.class_inc16(W, Gb) != ct.model_inc16(W, Gb):
                out.append((W, Gb, W * (Gb - Gb // 4)))          # 6, 12, 24 lanes per segment
    return out


def design(C, table):
    moved, edges = ct.moved_lengths(table)
    cells = changed_cells(table)
    lengths = sorted(set(moved) | set(edges) | {100, 650} | set(KNOB_LENGTHS) | {lb for _, _, lb in cells})
    cases = []
    for lb in lengths:
        nseg = C.task_shape(lb)["streams"]
        cases += [(lb, rows, False) for rows in sorted({1, nseg, nseg + 1, 40})]
        cases.append((lb, nseg + 1, True))
    return moved, cells, lengths, cases


@pytest.fixture(scope="module")
def collection(native_built):
    from oracle import oracle
    from phamclust_amd import hip
    from phamclust_amd.pack import pack_genomes
    table = ct.Table()
    moved, cells, lengths, cases = design(hip.Context, table)
    packed = pack_genomes(pc.build(cases, seed=10))
    want = {}
    for rule in (0, 3):
        oracle.set_tie_rule(rule)
        try:
            for metric in ("peq", "aai_ppos"):
                want[(metric, rule)] = oracle.fill(packed, metric, True)
        finally:
            oracle.set_tie_rule(0)
    print(f"{len(moved)} moved lengths, {len(cells)} classes of another cell, {len(lengths)} lengths in the collection, {len(cases)} buckets")
    return {"table": table, "moved": moved, "cells": cells, "lengths": lengths, "cases": cases, "packed": packed, "want": want,
            "count": pc.count(packed), "oracle": oracle}


def test_collection_covers_the_moved_classes(collection):
    """Every designed bucket is in the packed collection; EVERY moved length is in it with the length before and after its run, and runs on
    the table's variant, not the model's; every launch class of another cell has its length."""
    from phamclust_amd import hip
    C = hip.Context
    assert set(collection["cases"]) <= set(collection["count"]["buckets"])
    lengths, moved = set(collection["lengths"]), collection["moved"]
    assert moved and set(moved) <= lengths
    for lb in moved:
        assert {max(1, lb - 1), min(ct.MAX_LB, lb + 1)} <= lengths, lb
        assert C.variant_width(lb) == collection["table"].choice(lb) != ct.model_choice(lb), lb
    for lb in collection["lengths"]:
        assert C.variant_width(lb) == collection["table"].choice(lb)
    for W, Gb, lb in collection["cells"]:
        assert lb in lengths and ct.g_bucket(ct.lanes(lb, W)) == Gb, (W, Gb, lb)
    assert C.variant_width(100) == 13 and C.variant_width(650) == 32            # the pinned cases of tests/test_host.py


@pytest.mark.parametrize("rule", [0, 3])
def test_moved_classes_equal_the_oracle(gpu_ctx, collection, rule):
    saved = os.environ.pop("PC_PIPE", None)
    try:
        gpu_ctx.upload(collection["packed"])
        gpu_ctx.set_shard(0, 1)
        gpu_ctx.set_plan_budget(0)
        gpu_ctx.set_tie_rule(rule)
        for pipe in (None, "0"):
            if pipe is None:
                os.environ.pop("PC_PIPE", None)
            else:
                os.environ["PC_PIPE"] = pipe
            for metric in ("peq", "aai_ppos"):
                got = gpu_ctx.fill(metric, True)
                assert np.array_equal(got, collection["want"][(metric, rule)]), (metric, rule, pipe)
        tasks = gpu_ctx.last_plan_tasks()                                         # the device cut is the host cut, class by class
        want = pc.predict(type(gpu_ctx), collection["count"]["buckets"], len(tasks))
        assert np.array_equal(tasks, want), np.flatnonzero(tasks != want)[:12].tolist()
    finally:
        gpu_ctx.set_tie_rule(0)
        os.environ.pop("PC_PIPE", None)
        if saved is not None:
            os.environ["PC_PIPE"] = saved


@pytest.mark.parametrize("rule", [0, 3])
def test_classes_of_another_cell_equal_the_oracle(gpu_ctx, collection, rule):
    """Each (W, bucket) class whose cell the table changed, forced: the buckets of its length (1, nseg, nseg + 1, 40 rows of the chooser's
    variant -- on W they are other multiples of its segments) in the class's own workgroup and cut as a fill cuts them."""
    packed, count, O = collection["packed"], collection["count"], collection["oracle"]
    assert collection["cells"]
    a_all, b_all = count["row_gene"], count["column_gene"]
    col_len = np.diff(packed.seq_off)[b_all]
    gpu_ctx.upload(packed)
    gpu_ctx.set_tie_rule(rule)
    O.set_tie_rule(rule)
    try:
        for W, Gb, lb in collection["cells"]:
            pick = np.flatnonzero(col_len == lb)
            a, b = a_all[pick], b_all[pick]
            assert a.size >= 40
            _, want_ident, want_diag = O.nw_batch(packed.residues, packed.seq_off, a, b)
            for like_fill in (False, True):
                ident, diag = gpu_ctx.align_pairs(a, b, variant=W, like_fill=like_fill)
                assert np.array_equal(ident, want_ident) and np.array_equal(diag, want_diag), (W, Gb, lb, like_fill, rule)
    finally:
        O.set_tie_rule(0)
        gpu_ctx.set_tie_rule(0)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import json
import planner_cases as pc
from phamclust_amd import hip
from phamclust_amd.pack import pack_genomes
packed = pack_genomes(pc.build([tuple(case) for case in json.load(open(sys.argv[1]))], seed=10))
with hip.Context(0) as ctx:
    ctx.upload(packed)
    for metric in ("peq", "aai_ppos"):
        assert np.array_equal(ctx.fill(metric, True), np.load(sys.argv[2])[metric]), metric + " differs from the oracle"
    tasks = ctx.last_plan_tasks()
    want = pc.predict(hip.Context, pc.count(packed)["buckets"], len(tasks))              # the host cut under THIS process's switches
    assert np.array_equal(tasks, want), "device cut != host cut"
    print(json.dumps({"w650": hip.Context.variant_width(650), "w160": hip.Context.variant_width(160), "waves700": hip.Context.task_shape(700, 11)["waves"]}))
'''


def test_switches_in_child_processes(native_built, collection):
    """PC_RATE_TABLE=0 / 1 / 2, PC_CHOOSE_MAX_W=24 and PC_INC16=2 are policy (read once per process: children, three at a time): each gives
    the oracle's peq and percent-positives matrices of the collection and a device cut equal to the host cut made under the same switch --
    and each does switch something."""
    from phamclust_amd import hip
    here = os.path.dirname(os.path.abspath(__file__))
    settings = (("default", {}), ("table_off", {"PC_RATE_TABLE": "0"}), ("variant_only", {"PC_RATE_TABLE": "1"}), ("cell_only", {"PC_RATE_TABLE": "2"}),
                ("max_w24", {"PC_CHOOSE_MAX_W": "24"}), ("inc16_fits", {"PC_INC16": "2"}))
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        cases, want = os.path.join(tmp, "cases.json"), os.path.join(tmp, "want.npz")
        json.dump(collection["cases"], open(cases, "w"))
        np.savez(want, peq=collection["want"][("peq", 0)], aai_ppos=collection["want"][("aai_ppos", 0)])
        code = CHILD % (os.path.dirname(here), here)
        for wave in (settings[:3], settings[3:]):
            procs = [(name, subprocess.Popen([sys.executable, "-c", code, cases, want], env=dict(os.environ, PHAMCLUST_NO_TORCH="1", **env),
                                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for name, env in wave]
            for name, proc in procs:
                out, err = proc.communicate(timeout=300)
                assert proc.returncode == 0, (name, out[-1500:], err[-3000:])
                seen[name] = json.loads(out.strip().splitlines()[-1])
    assert seen["default"]["w650"] == 32 and seen["max_w24"]["w650"] == 11
    assert seen["default"]["w160"] == collection["table"].choice(160) != ct.model_choice(160) == seen["table_off"]["w160"] == seen["cell_only"]["w160"]
    assert seen["default"]["waves700"] == 4 and seen["inc16_fits"]["waves700"] == 8       # W = 11 on 64 lanes: the profile cell takes 8-wave workgroups
