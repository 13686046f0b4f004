"""The kernels of the distribution fill on injected pair values (GPU): one value in every pair (64 lanes on one address, the empty
marker against key 0), values that all differ (more keys per chunk than the workgroup's table holds: the overflow path), keys that
share one probe run, chunk and slab seams, partitions, the rows form with poisoned dead elements and its seed refusals, several
contexts, and the refusals of values that are no millionth in [0, 1] -- device code no genome collection can reach.

The values go in through ``hip.set_slab_values`` / ``hip.set_rows_values``, which exist only in the test-hooks twin of the library, and
the variant is chosen when ``phamclust_amd.hip`` is imported: every case runs in a child process, tests/hist_values_driver.py <case>,
one at a time and under its own time limit.  The child compares integer for integer with the references of tests/hist_value_cases.py,
which tests/test_distribution_host.py holds to ``PairDistribution.from_dense``; it prints ``ok <case> <comparisons>``.  If a child ends
by a signal, by its time limit or on a failed HIP runtime call (PC_ERR_HIP), the cases after it fail at once without starting another."""

import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(REPO, "tests", "hist_values_driver.py")
LIMIT = 120
CASES = ["hot", "distinct", "collide", "seams", "partition", "rows", "multi", "refusals"]
_broken = []                           # the case whose child was killed: what it ran may have faulted, nothing more is started


def test_the_cases_are_the_drivers():
    import ast
    tree = ast.parse(open(DRIVER).read())
    named = next(node for node in ast.walk(tree) if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "CASES")
    assert [key.value for key in named.value.keys] == CASES


@pytest.mark.parametrize("case", CASES)
def test_hist_values(native_built, case):
    if _broken:
        pytest.fail(f"not started: the child of case '{_broken[0]}' ended by a signal, by its time limit or on a failed HIP call")
    env = dict(os.environ, PHAMCLUST_NATIVE_VARIANT="hooks", PHAMCLUST_NO_TORCH="1")
    try:
        run = subprocess.run([sys.executable, DRIVER, case], env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired as exc:
        _broken.append(case)
        pytest.fail(f"case '{case}' ran into its time limit of {LIMIT} s:\n{exc.stdout}")
    if run.returncode < 0 or (run.returncode != 0 and "status -2" in run.stdout):      # a signal, or a HIP runtime call that failed
        _broken.append(case)
    assert run.returncode == 0, f"case '{case}' ended with status {run.returncode}:\n{run.stdout[-4000:]}"
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[:2] == ["ok", case] and int(last[2]) > 0, run.stdout[-4000:]
