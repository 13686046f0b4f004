"""The fill's device-side planner (pc_plan.hip and the per-sequence tables pc_upload_residues builds) over every launch class
it can choose (run with ``-m gpu``).

pc_align_pairs, which nearly every aligner test goes through, cuts its buckets on the host.  Here one designed collection
(tests/planner_cases.py: column lengths on both sides of every variant and lanes-per-segment change up to 4,096 residues and
beyond the strip-mined variants' 64 x W columns, each with bucket sizes around nseg, the remainder chooser's moves and the task
size, clean and with a byte outside the alphabet) goes through pc_fill itself.  tests/test_host.py proves on the CPU that its
buckets reach every launch class a default process can reach.  The values are held to the oracle bit for bit, the device cut
(pc_last_plan_tasks) to the host cut (pc_bucket_launch_classes) class by class, the counters to a recount in numpy, on every
route a fill can take: one piece, chunks, shards, alignment slices, and the launch-policy switches in processes of their own.

Measured with 16 cores beside an MI355X: 57 s for the module -- 27 s building, packing and recounting the collection (262,517 phams,
1.5 x 10^9 DP cells), 15 s for the oracle's five matrices (each computed once), the rest uploads, fills and the child processes.
"""

import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import planner_cases as pc

pytestmark = pytest.mark.gpu


class Collection:
    def __init__(self):
        from oracle import oracle
        from phamclust_amd import hip
        from phamclust_amd.pack import pack_genomes
        self.O, self.C = oracle, hip.Context
        self.cases = pc.design(self.C)
        self.packed = pack_genomes(pc.build(self.cases))
        self.count = pc.count(self.packed)
        self.oracle_seconds = 0.0
        self._want = {}

    def want(self, metric, as_distance=True, rule=0):
        """The oracle's matrix, computed once per (metric, direction, tie rule) and reused by every route."""
        key = (metric, bool(as_distance), rule)
        if key not in self._want:
            t0 = time.time()
            self.O.set_tie_rule(rule)
            try:
                self._want[key] = self.O.fill(self.packed, metric, as_distance)
            finally:
                self.O.set_tie_rule(0)
            self.oracle_seconds += time.time() - t0
            print(f"oracle {metric} rule {rule}: {time.time() - t0:.1f} s (oracle total {self.oracle_seconds:.1f} s)")
        return self._want[key]

    def predicted(self, n_classes, group_of_target=None):
        """Tasks per launch class by the host cut, the targets planned group by group (default: all at once)."""
        groups = {0: self.count["buckets"]} if group_of_target is None else pc.buckets_by_group(self.count, group_of_target)
        return sum((pc.predict(self.C, b, n_classes) for b in groups.values()), np.zeros(n_classes, dtype=np.int64))


@pytest.fixture(scope="module")
def collection(native_built):
    return Collection()


@pytest.fixture()
def ctx(gpu_ctx, collection):
    gpu_ctx.upload(collection.packed)
    gpu_ctx.set_shard(0, 1)
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_tie_rule(0)
    os.environ.pop("PC_PIPE", None)
    yield gpu_ctx
    os.environ.pop("PC_PIPE", None)
    gpu_ctx.set_tie_rule(0)
    gpu_ctx.set_plan_budget(0)
    gpu_ctx.set_shard(0, 1)


def test_the_collection_is_the_design(collection):
    """Every designed case is a bucket of the packed collection -- same column length, row count and any-byte flag -- and what
    else is there (paralog, tie and shared phams) adds small buckets only."""
    from collections import Counter
    extra = Counter(collection.count["buckets"])
    extra.subtract(Counter(collection.cases))
    assert min(extra.values()) >= 0, [case for case, n in extra.items() if n < 0][:10]
    assert all(lb <= 400 and rows <= 16 for (lb, rows, _), n in extra.items() if n > 0)
    assert collection.count["n_alignments"] > collection.count["n_distinct_alignments"] > 250000


def test_fills_equal_the_oracle(ctx, collection):
    """aai, peq (distance and similarity) and percent-positives of the whole collection, bit for bit; the strip-mined launches
    one row per wave (PC_PIPE=0, read per launch) and as the launcher chooses; peq once more under tie rule 3."""
    for metric, as_distance in (("aai", True), ("peq", True), ("peq", False), ("aai_ppos", True)):
        got, st = ctx.fill(metric, as_distance, want_stats=True)
        assert st["n_chunks"] == 1
        assert np.array_equal(got, collection.want(metric, as_distance)), (metric, as_distance)
    for rule in (0, 3):
        ctx.set_tie_rule(rule)
        for pipe in ("0", None):
            if pipe is None: os.environ.pop("PC_PIPE", None)
            else: os.environ["PC_PIPE"] = pipe
            assert np.array_equal(ctx.fill("peq"), collection.want("peq", True, rule)), (rule, pipe)


def test_device_cut_equals_host_cut(ctx, collection):
    """pc_last_plan_tasks of the one-piece fill == the tasks pc_bucket_launch_classes predicts for the collection's buckets, launch
    class by launch class; their sum is stats.n_tasks; every class the CPU coverage test promises is really reached."""
    from phamclust_amd import hip
    with hip.Context(0) as fresh:
        with pytest.raises(hip.HipLibraryError):
            fresh.last_plan_tasks()                                          # no fill yet
    for metric in ("peq", "aai_ppos"):                                       # (percent-positives swaps kernels, not the cut)
        _, st = ctx.fill(metric, want_stats=True)
        tasks = ctx.last_plan_tasks()
        want = collection.predicted(len(tasks))
        differ = np.flatnonzero(tasks != want)
        assert differ.size == 0, [(int(c), pc.class_name(collection.C, int(c)), int(tasks[c]), int(want[c])) for c in differ[:12]]
        assert int(tasks.sum()) == st["n_tasks"]
    promised = pc.classes_of(collection.C, collection.cases)
    assert set(promised) <= set(np.flatnonzero(tasks).tolist())
    print(f"{len(np.flatnonzero(tasks))} launch classes reached, {int(tasks.sum())} tasks")


def test_any_byte_column_whose_main_variant_takes_any_byte(gpu_ctx, collection):
    """Named case (found by test_device_cut_equals_host_cut): a column of 641 ... 672 residues runs on W = 32, which compares
    residues and so keeps "any byte" columns in its ordinary class -- but the left-over rows of its three-row wave round go to
    W = 11, which has a profile cell: their task belongs to W = 11's "any byte" class.  The upload's remainder table kept the clean
    class for such columns while pc_align_pairs' host cut chose the "any byte" one."""
    from phamclust_amd.pack import pack_genomes
    C = collection.C
    cases = [(650, 4, True), (641, 5, True), (672, 7, True), (650, 4, False)]
    assert all(C.bucket_launch_classes(*case)["rem"] >= 0 for case in cases)
    packed = pack_genomes(pc.build(cases, seed=7))
    ct = pc.count(packed)
    got, st = gpu_ctx.upload(packed).fill("peq", want_stats=True)
    assert np.array_equal(got, collection.O.fill(packed, "peq"))
    tasks = gpu_ctx.last_plan_tasks()
    assert np.array_equal(tasks, pc.predict(C, ct["buckets"], len(tasks)))
    for lb, rows, any_byte in cases:                                         # W = 11 is variant 9, 59 ... 62 lanes: bucket <= 64
        rem = C.bucket_launch_classes(lb, rows, any_byte)["rem"]
        assert rem // 3 == 9 * 4 + 3 + (24 * 4 if any_byte else 0) and tasks[rem] > 0


def test_counters_equal_a_recount(ctx, collection):
    """n_alignments, n_distinct_alignments, n_cells, n_distinct_cells of the one-piece fill == the numpy recount over the
    packed genomes (anchor rule, distinct (row bytes, column bytes) pairs)."""
    for metric in ("aai", "peq"):
        _, st = ctx.fill(metric, want_stats=True)
        for name in ("n_alignments", "n_distinct_alignments", "n_cells", "n_distinct_cells"):
            assert st[name] == collection.count[name], (metric, name)
        assert st["n_pairs"] == collection.packed.n_pairs


def test_chunked_fills(ctx, collection):
    """A plan budget below one target's alignments (one target per chunk) and one of a fifth of the fill (3 ... 10 chunks): the
    oracle's matrix again; the chunks are where pc_chunk_plan puts them; the tasks of all chunks, class by class, are the host
    cut of each chunk's own buckets (duplicates merge inside a chunk only)."""
    per_target = collection.count["per_target"]
    total = collection.count["n_alignments"]
    seen = []
    for max_alignments in (1, (total + 4) // 5):
        ctx.set_plan_budget(56 * max_alignments)                              # 56 bytes of plan buffers per alignment
        cuts = collection.C.chunk_plan(per_target, max_alignments)
        group = np.repeat(np.arange(len(cuts) - 1), np.diff(cuts))
        for metric in ("peq", "aai"):
            got, st = ctx.fill(metric, want_stats=True)
            assert np.array_equal(got, collection.want(metric)), (metric, max_alignments)
            assert st["n_chunks"] == len(cuts) - 1, (st["n_chunks"], cuts)
            tasks = ctx.last_plan_tasks()
            assert np.array_equal(tasks, collection.predicted(len(tasks), group)) and int(tasks.sum()) == st["n_tasks"]
            assert st["n_alignments"] == total and st["n_cells"] == collection.count["n_cells"]
        seen.append(len(cuts) - 1)
    assert seen[0] >= pc.N_TARGETS and 3 <= seen[1] <= 10, seen


@pytest.mark.parametrize("balanced", [False, True])
def test_three_rank_shards(ctx, collection, balanced):
    """The shards of a 3-rank deal, plain and cost-balanced, assembled on the device: the oracle's matrix; each rank's tasks are the
    host cut of the buckets of the targets it owns."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    world, parts, reached = 3, [], set()
    for rank in range(world):
        ctx.set_shard(rank, world, balanced=balanced)
        t_rank, _ = ctx.shard_table()
        buf = torch.full((ctx.shard_stride(),), -1.0, dtype=torch.float64, device="cuda:0")
        st = ctx.fill_shard_dev("peq", True, buf.data_ptr(), stream)
        torch.cuda.synchronize()
        parts.append(buf)
        tasks = ctx.last_plan_tasks()
        want = collection.predicted(len(tasks), np.where(t_rank == rank, 0, -1))
        assert np.array_equal(tasks, want) and int(tasks.sum()) == st["n_tasks"], rank
        reached |= set(np.flatnonzero(tasks).tolist())
    gathered = torch.cat(parts)
    out = torch.empty(collection.packed.n_pairs, dtype=torch.float64, device="cuda:0")
    ctx.assemble_dev(gathered.data_ptr(), world, out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), collection.want("peq"))
    assert set(pc.classes_of(collection.C, collection.cases)) <= reached      # (a designed bucket lies behind ONE target: whole in one shard)


def test_alignment_sliced_route(ctx, collection):
    """plan_dev / three slices / reduce_dev: the oracle's matrix; pc_last_plan_tasks is the whole plan's counts after the plan and
    each slice's own after its alignment -- every world-th task of a class -- and the slices add up to the plan."""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    world = 3
    for metric in ("peq", "aai"):
        plan = ctx.plan_dev(metric, stream)
        whole = ctx.last_plan_tasks()
        assert np.array_equal(whole, collection.predicted(len(whole))) and int(whole.sum()) == plan["n_tasks"]
        n = plan["n_distinct_alignments"]
        assert n == collection.count["n_distinct_alignments"]
        total, summed = torch.zeros(n, dtype=torch.int64, device="cuda"), np.zeros_like(whole)
        for rank in range(world):
            res = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            ctx.align_slice_dev(rank, world, res.data_ptr(), stream)
            mine = ctx.last_plan_tasks()
            assert np.array_equal(mine, (np.maximum(whole - rank, 0) + world - 1) // world), rank
            summed += mine
            total += res
        torch.cuda.synchronize()
        assert np.array_equal(summed, whole)
        out = torch.empty(collection.packed.n_pairs, dtype=torch.float64, device="cuda")
        ctx.reduce_dev(metric, True, total.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), collection.want(metric)), metric


def test_align_pairs_over_every_distinct_alignment(ctx, collection):
    """The HOST cut on the same buckets: pc_align_pairs (automatic variant) over every distinct alignment of the collection, the
    rows of a column sequence against ONE gene that carries it, gives the oracle's (n_ident, n_diag).  Should the fills above
    fail and this pass, the device planner is at fault; the other way round, the host cut."""
    a, b = collection.count["row_gene"], collection.count["column_gene"]
    ident, diag = ctx.align_pairs(a, b, variant=0)
    t0 = time.time()
    _, want_ident, want_diag = collection.O.nw_batch(collection.packed.residues, collection.packed.seq_off, a, b)
    collection.oracle_seconds += time.time() - t0
    assert np.array_equal(ident, want_ident) and np.array_equal(diag, want_diag)


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import planner_cases as pc
from phamclust_amd import hip
from phamclust_amd.pack import pack_genomes
C = hip.Context
packed = pack_genomes(pc.build([tuple(case) for case in json.load(open(sys.argv[2]))]))
with C(0) as ctx:
    ctx.upload(packed)
    got, st = ctx.fill("peq", want_stats=True)
    assert np.array_equal(got, np.load(sys.argv[1])), "peq differs from the oracle"
    tasks = ctx.last_plan_tasks()
    buckets = [tuple(b) for b in json.load(open(sys.argv[3]))]
    want = pc.predict(C, buckets, len(tasks))                  # the host cut under THIS process's switches
    assert np.array_equal(tasks, want), "device cut != host cut: " + str(np.flatnonzero(tasks != want)[:12].tolist())
    moved = sum(C.bucket_launch_classes(*b)["rem"] >= 0 for b in buckets)
    unmoved = sum(-(-b[1] // C.bucket_launch_classes(*b)["per"]) for b in buckets)
    print(json.dumps({"tasks": int(tasks.sum()), "n_tasks": st["n_tasks"], "small_mode_tasks": int(tasks.reshape(-1, 3)[:, 1:].sum()),
                      "moved_remainders": int(moved), "tasks_without_moves": int(unmoved), "launches": st["n_align_launches"]}))
'''


def test_policy_switches_in_child_processes(native_built, collection):
    """PC_REMAINDER=0, PC_SMALL_MODES=0, PC_FUSE=0 with PC_SMALL_LAUNCH_MIN=1, PC_INC16=0 / 1 and a quarter of the task budget
    are policy: each gives the oracle's peq matrix, and in each the device cut equals the host cut made under the same switch.
    Without the remainder chooser no task is a remainder task; without the small modes every task runs in its class's workgroup.
    (The switches are read once per process: children, three at a time.)"""
    here = os.path.dirname(os.path.abspath(__file__))
    settings = (("default", {}), ("no_remainder", {"PC_REMAINDER": "0"}), ("no_small_modes", {"PC_SMALL_MODES": "0"}),
                ("per_class", {"PC_FUSE": "0", "PC_SMALL_LAUNCH_MIN": "1"}), ("inc16_off", {"PC_INC16": "0"}), ("inc16_on", {"PC_INC16": "1"}),
                ("quarter_budget", {"PC_TASK_BUDGET": str(49152 // 4)}))
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        want, cases, buckets = (os.path.join(tmp, name) for name in ("want.npy", "cases.json", "buckets.json"))
        np.save(want, collection.want("peq"))
        json.dump(collection.cases, open(cases, "w"))
        json.dump(collection.count["buckets"], open(buckets, "w"))
        code = CHILD % (os.path.dirname(here), here)
        for wave in (settings[:3], settings[3:6], settings[6:]):
            procs = [(name, subprocess.Popen([sys.executable, "-c", code, want, cases, buckets], env=dict(os.environ, PHAMCLUST_NO_TORCH="1", **env),
                                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for name, env in wave]
            for name, proc in procs:
                out, err = proc.communicate(timeout=600)
                assert proc.returncode == 0, (name, out[-1500:], err[-3000:])
                seen[name] = json.loads(out.strip().splitlines()[-1])
    for name, s in seen.items():
        assert s["tasks"] == s["n_tasks"] > 0, (name, s)
    d = seen["default"]
    assert d["moved_remainders"] > 1000 and d["small_mode_tasks"] > 1000
    assert seen["no_remainder"]["moved_remainders"] == 0 and seen["no_remainder"]["tasks"] == seen["no_remainder"]["tasks_without_moves"]
    assert seen["no_small_modes"]["small_mode_tasks"] == 0 and seen["no_small_modes"]["tasks"] == d["tasks"]
    assert seen["per_class"]["tasks"] == d["tasks"] and seen["per_class"]["launches"] > d["launches"]
    assert seen["quarter_budget"]["tasks"] > d["tasks"]
    print("policy switches:", seen)

