"""The variant, cell and remainder choosers of pc_nw_shape.hip against the rate table they were compiled with (pc_nw_rates.h, written from
profiles/r10/class_rates.json): for every column length 1 ... 1,536, through Context.task_shape and bucket_launch_classes, no GPU.

* the chosen class is launchable: at most 64 lanes per segment, the LDS launch_shape asks for at most a CU's 160 KB in every
  launch mode and for percent-positives, and a class's own workgroup holds a full task;
* the choice is the table's argmin under the hysteresis rule, against the brute-force mirror of tests/chooser_table_cases.py;
* no length goes to a variant that cannot hold it, main task or remainder.
"""

import re

import pytest

import chooser_table_cases as ct

LENGTHS = range(1, ct.MAX_LB + 1)
NVAR = len(ct.VARIANTS)


@pytest.fixture(scope="module")
def table(native_built):
    return ct.Table()


def _decode(cls):
    """launch class -> (columns per lane, lanes-per-segment bucket, any-byte class, mode)"""
    base, mode = divmod(cls, 3)
    assert 0 <= base < NVAR * 8, cls
    any_byte, base = divmod(base, NVAR * 4)
    return ct.VARIANTS[base // 4], 8 << (base % 4), bool(any_byte), mode


def test_header_is_the_record(table):
    """The compiled table is the record's: the header names the record file and its device-code hash and holds its 64-row points."""
    src = open(ct.REPO + "/phamclust_amd/csrc/pc_nw_rates.h").read()
    rows = re.findall(r"^\s*\{(\d+), (\d+), (\d+), ([0-9.]+)f, ([0-9.]+)f\},", src, re.M)
    assert [(int(w), int(c), int(g), float(s), float(e)) for w, c, g, s, e in rows if int(w)] == \
        [(w, c, g, float(f"{s:.4f}"), float(f"{e:.4f}")) for w, c, g, s, e in table.points]
    pins = [(int(a), int(b)) for a, b in re.findall(r"^\s*\{(\d+), (\d+)\},", src, re.M) if (int(a), int(b)) != (0, 0)]
    assert pins == table.pins
    if table.points:
        assert "profiles/r10/class_rates.json" in src and table.hash in src


def test_chosen_classes_are_launchable(table):
    from phamclust_amd import hip
    C = hip.Context
    for lb in LENGTHS:
        W = C.variant_width(lb)
        shape = C.task_shape(lb)
        G = ct.lanes(lb, W)
        assert 1 <= G <= 64, (lb, W)
        assert shape["streams"] == ct.nseg_of(G) and shape["passes"] == 0
        assert shape["waves"] == table.waves(W, G), (lb, W, shape)
        assert shape["waves"] >= 4 and shape["waves"] * 52 >= shape["rows"], (lb, shape)         # a class's own workgroup holds a full task
        for mode in (0, 1, 2):
            for compare_only in (False, True):
                nw, _, lds = table.launch_lds(W, lb, mode, compare_only=compare_only)
                assert lds <= ct.LDS_PER_CU, (lb, W, mode, compare_only, nw, lds)
        pw = C.ppos_width(lb)                                                                     # percent-positives: the profile cell
        assert 0 < pw <= ct.INC16_MAX_W and ct.lanes(lb, pw) <= 64
        for mode in (0, 1, 2):
            nw, inc16, lds = table.launch_lds(pw, lb, mode, ppos=True)
            assert inc16 and lds <= ct.LDS_PER_CU, (lb, pw, mode, nw, lds)


def test_choice_is_the_tables_argmin_under_hysteresis(table):
    from phamclust_amd import hip
    C = hip.Context
    differ = [(lb, C.variant_width(lb), table.choice(lb)) for lb in LENGTHS if C.variant_width(lb) != table.choice(lb)]
    assert not differ, differ[:10]
    for lb in LENGTHS:                                       # a pinned length, and one the record does not price, keeps the model's
        if table.pinned(lb) or table.rate_of(ct.model_choice(lb), lb) is None:
            assert C.variant_width(lb) == ct.model_choice(lb), lb


def test_no_length_goes_to_a_variant_that_cannot_hold_it(table):
    from phamclust_amd import hip
    C = hip.Context
    for lb in LENGTHS:
        W = C.variant_width(lb)
        nseg = ct.nseg_of(ct.lanes(lb, W))
        cell_bucket = ct.g_bucket(ct.lanes(lb, W))
        for rows in sorted({1, nseg, nseg + 1, 2 * nseg - 1 if nseg > 1 else 2, 40, 64}):
            for any_byte in (False, True):
                cut = C.bucket_launch_classes(lb, rows, any_byte)
                for name in ("full", "last", "rem"):
                    if cut[name] < 0:
                        continue
                    w, bucket, odd, mode = _decode(cut[name])
                    assert ct.lanes(lb, w) <= 64 and bucket == ct.g_bucket(ct.lanes(lb, w)), (lb, rows, name, w)
                    assert odd == (any_byte and w <= ct.INC16_MAX_W), (lb, rows, name)
                    if name != "rem":
                        assert w == W and bucket == cell_bucket
                r = rows % nseg if nseg > 1 else 0
                want = table.remainder(lb, r, W) if r else None
                assert (cut["rem"] < 0) == (want is None), (lb, rows, cut, want)
                if want is not None:
                    assert _decode(cut["rem"])[0] == want and cut["n_main"] == rows - r, (lb, rows, cut, want)
