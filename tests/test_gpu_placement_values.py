"""The kernels of the rows form of the affinity fill on injected row values (GPU): k_aff_qrows, k_aff_qcols and k_aff_qfinish at N = 2, 3,
63 .. 65, 255 .. 257 and 513 with G = 1, 3, 64, 65 and 2,048 -- runs of 70 consecutive columns of one group (the wave-uniform path) with
the diagonal and a -1 label inside, alternating labels (the ds-atomic path), scattered labels that leave most groups empty; queries at
both ends and adjacent, a labelled pair of them inside one 64-column block; the values 0, -0.0 and 10^6, a sum above 2^32, ties between
groups under all three criteria; a NaN on the diagonal and in every column of an unlabelled genome, which no pass may read; and refused
values, counted once per pair.  Device code that a genome collection cannot reach with values of its own.

The values go in through ``hip.set_rows_values``, which exists only in the test-hooks twin of the library, and the variant is chosen
when ``phamclust_amd.hip`` is imported: every case runs in a child process, tests/placement_values_driver.py <case>, one at a time.  The
child compares exactly with ``GroupPlacement.from_dense`` of tests/placement_value_cases.py's inputs, which tests/test_placement_host.py
holds to plain loops; it prints ``ok <case> <comparisons>``.  If a child ends by a signal, by its time limit or on a failed HIP runtime
call (PC_ERR_HIP), the cases after it fail at once without starting another."""

import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(REPO, "tests", "placement_values_driver.py")
LIMIT = 120
CASES = ["tiny", "n63", "n64", "n65", "n255", "n256", "n257", "n513", "wide", "refusals"]
_broken = []                           # the case whose child was killed: what it ran may have faulted, nothing more is started


def test_the_cases_are_the_drivers():
    import ast
    tree = ast.parse(open(DRIVER).read())
    named = next(node for node in ast.walk(tree) if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "CASES")
    assert [key.value for key in named.value.keys] == CASES


@pytest.mark.parametrize("case", CASES)
def test_placement_values(native_built, case):
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
