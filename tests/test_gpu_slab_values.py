"""The kernels of the slab fills on injected pair values (GPU): ties with random structure, elements that all differ at the shapes
where a misattributed value would otherwise change no sum, multi-group ranges of the affinity fill's column pass, and the refusals
of values that are no millionth in [0, 1] -- device code no genome collection can reach.

The values go in through ``hip.set_slab_values``, which exists only in the test-hooks twin of the library, and the variant is chosen
when ``phamclust_amd.hip`` is imported: every case runs in a child process, tests/slab_values_driver.py <case>, one at a time.  The
child compares exactly (integers, or the uint64 view of values) with the references of tests/slab_value_cases.py, which
tests/test_slab_values_host.py holds to the host statements; it prints ``ok <case> <comparisons>``.  If a child ends by a signal, by
its time limit or on a failed HIP runtime call (PC_ERR_HIP), the cases after it fail at once without starting another."""

import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(REPO, "tests", "slab_values_driver.py")
DEFAULT_LIMIT = 120
# (case, time limit in seconds): the two large shapes pack thousands of genomes and run their references on millions of pairs
CASES = [("tree", DEFAULT_LIMIT), ("tree_tiny", DEFAULT_LIMIT), ("components_edges_130", DEFAULT_LIMIT), ("components_edges_515", 240),
         ("components_edges_finite", DEFAULT_LIMIT), ("nearest", DEFAULT_LIMIT), ("between", DEFAULT_LIMIT), ("between_segment", 300),
         ("affinity", DEFAULT_LIMIT), ("affinity_mean_tie", DEFAULT_LIMIT), ("affinity_ranges", 300), ("multi", DEFAULT_LIMIT),
         ("refusals", DEFAULT_LIMIT)]
_broken = []                           # the case whose child was killed: what it ran may have faulted, nothing more is started


def test_the_cases_are_the_drivers():
    import ast
    tree = ast.parse(open(DRIVER).read())
    named = next(node for node in ast.walk(tree) if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "CASES")
    assert [key.value for key in named.value.keys] == [case for case, _ in CASES]


@pytest.mark.parametrize("case,limit", CASES, ids=[case for case, _ in CASES])
def test_slab_values(native_built, case, limit):
    if _broken:
        pytest.fail(f"not started: the child of case '{_broken[0]}' ended by a signal, by its time limit or on a failed HIP call")
    env = dict(os.environ, PHAMCLUST_NATIVE_VARIANT="hooks", PHAMCLUST_NO_TORCH="1")
    try:
        run = subprocess.run([sys.executable, DRIVER, case], env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    except subprocess.TimeoutExpired as exc:
        _broken.append(case)
        pytest.fail(f"case '{case}' ran into its time limit of {limit} s:\n{exc.stdout}")
    if run.returncode < 0 or (run.returncode != 0 and "status -2" in run.stdout):      # a signal, or a HIP runtime call that failed
        _broken.append(case)
    assert run.returncode == 0, f"case '{case}' ended with status {run.returncode}:\n{run.stdout[-4000:]}"
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[:2] == ["ok", case] and int(last[2]) > 0, run.stdout[-4000:]
