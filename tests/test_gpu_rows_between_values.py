"""The kernel of the rows form of the between-groups fill, k_between_qrows, on injected row values (GPU): N = 2, 3, 63 .. 65, the seam of
PC_BETWEEN_SEGMENT at 4,095 .. 4,097 (an odd N puts every second row at an odd start: the paired load's alignment rule), 8,193 (three
segments), with 1 .. 3 query rows and once with all rows -- one group (whole waves of one group: the reduction), two alternating groups
(split lanes), 2,048 groups on N = 4,097, a group held only by queries, labels of -1; values that all differ, random ties, 0.0, -0.0 and
1.0; the diagonal, the dead copy of a pair of two queries and everything of an unlabelled genome poisoned with 0.5 (which no live
element holds) and 2.0 (which would fail the call if a pass checked it); a live 2.0 and a live 0.1234565, refused with their count; and
seeds that satisfy nothing but the contract.  Device code that a genome collection, whose rows slab is a symmetric matrix's, cannot reach.

The values go in through ``hip.set_rows_values``, which exists only in the test-hooks twin of the library, and the variant is chosen
when ``phamclust_amd.hip`` is imported: every case runs in a child process, tests/rows_between_values_driver.py <case>, one at a time.
The child compares exactly with the plain loops of tests/rows_between_value_cases.py, which tests/test_rows_between_host.py holds to
``GroupLinkage.extended``; it prints ``ok <case> <comparisons>``.  If a child ends by a signal, by its time limit or on a failed HIP
runtime call (PC_ERR_HIP), the cases after it fail at once without starting another."""

import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(REPO, "tests", "rows_between_values_driver.py")
LIMIT = 120
CASES = ["tiny", "n63", "n64", "n65", "n65_all", "n4095", "n4096", "n4097", "n8193", "many_groups", "refusals"]
_broken = []                           # the case whose child was killed: what it ran may have faulted, nothing more is started


def test_the_cases_are_the_drivers():
    import ast
    tree = ast.parse(open(DRIVER).read())
    named = next(node for node in ast.walk(tree) if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "CASES")
    assert [key.value for key in named.value.keys] == CASES


@pytest.mark.parametrize("case", CASES)
def test_rows_between_values(native_built, case):
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
