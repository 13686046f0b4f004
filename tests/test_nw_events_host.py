"""The flag-event schedule of the systolic kernel's step loop (phamclust_amd/csrc/pc_nw_events.h) on the CPU: the header is plain
integer arithmetic, so a stand-alone program (tests/nw_events_check.cpp, own main) replays a wave's windows and steps around it and
compares every step's RESET / LAST answer with a brute-force list of (step, event): every output lane k_out = 0 ... 63, row lengths
1 ... 70, streams of 1 ... 5 rows, 1, 2 and 16 segments, empty streams, up to twelve consecutive windows.  Built with
-fsanitize=address,undefined: a shift by 64 or more in the 128-bit placement would be undefined behaviour, and is reported as such.
"""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_event_schedule_matches_brute_force(tmp_path):
    exe = str(tmp_path / "nw_events_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "phamclust_amd", "csrc"),
                           os.path.join(ROOT, "tests", "nw_events_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    m = re.search(r"cases (\d+) events (\d+) max_windows (\d+) mismatches 0", p.stdout)
    assert m, p.stdout[-1000:]
    assert int(m.group(1)) >= 64 * (70 * 5 + 3 * 40) and int(m.group(2)) > 0 and int(m.group(3)) >= 4
