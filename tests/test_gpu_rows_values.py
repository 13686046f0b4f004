"""The kernels of the rows forms on injected row values (GPU): the rows instance of every flat pass body (PcRowsDomain: edge count and
emit, the union, the tree scan) at the row ends, strides and carries of n = 2, 3, 63 .. 65, 511 .. 513 and 4,099, the two rows passes of
the nearest fill (k_nn_qrows, k_nn_qcols) around their 16-column and 64-column seams, and the three seeds where they satisfy nothing but
their contract -- on values that all differ, on random ties, on the two zeros, subnormals and values one ulp apart, and on slabs whose
diagonal and dead duplicates hold a value that would change the result if a kernel read it.  Device code that a genome collection, whose
rows slab is a symmetric matrix's, cannot reach.

The values go in through ``hip.set_rows_values``, which exists only in the test-hooks twin of the library, and the variant is chosen
when ``phamclust_amd.hip`` is imported: every case runs in a child process, tests/rows_values_driver.py <case>, one at a time.  The
child compares exactly (integers, or the uint64 view of values) with the references of tests/rows_value_cases.py, which
tests/test_rows_values_host.py holds to the host statements; it prints ``ok <case> <comparisons>``.  If a child ends by a signal, by
its time limit or on a failed HIP runtime call (PC_ERR_HIP), the cases after it fail at once without starting another."""

import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(REPO, "tests", "rows_values_driver.py")
LIMIT = 120
CASES = ["flat_tiny", "flat_63", "flat_64", "flat_65", "flat_511", "flat_512", "flat_513", "flat_wide", "grow", "nearest_tiny", "nearest_64",
         "nearest_65", "nearest_129", "nearest_130", "refusals"]
_broken = []                           # the case whose child was killed: what it ran may have faulted, nothing more is started


def test_the_cases_are_the_drivers():
    import ast
    tree = ast.parse(open(DRIVER).read())
    named = next(node for node in ast.walk(tree) if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "CASES")
    assert [key.value for key in named.value.keys] == CASES


@pytest.mark.parametrize("case", CASES)
def test_rows_values(native_built, case):
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
