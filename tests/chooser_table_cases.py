"""A brute-force mirror in Python of the choosers of pc_nw_shape.hip (variant, cell, remainder) and of its launch arithmetic, reading the
same numbers the library was compiled with from profiles/r10/class_rates.json (no GPU call here).  tests/test_chooser_table_host.py
holds the library to it for every column length; tests/test_gpu_chooser_refit.py takes from it the lengths at which the table moved
a choice.

The model: the r01-r04 cost fit, "today's choice" -- what a length the record does not price keeps, and what a priced variant has
to beat by more than the spread of the two points.
"""

import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(REPO, "profiles", "r10", "class_rates.json")
VARIANTS = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 24, 32, 48, 64]
INC16_MAX_W, MAX_SEG, WIN, MAX_LB = 24, 16, 32, 1536
LDS_PER_CU = 160 * 1024


def nseg_of(G):
    return min(64 // G, MAX_SEG)


def g_bucket(G):
    return 8 if G <= 8 else 16 if G <= 16 else 32 if G <= 32 else 64


def lanes(lb, W):
    return -(-lb // W)


def lds_bytes(W, G, nw, inc16, any_bucket=False):
    """systolic_lds_bytes: score table, the waves' private regions, the profile"""
    Gb = g_bucket(G)
    rpl = 64 // Gb
    nseg_max = MAX_SEG if Gb == 8 or any_bucket else min(64 // (Gb // 2 + 1), MAX_SEG)
    prof_rows = 25 if inc16 else 24
    row_dwords = (W + 3) // 4 + ((W + 1) // 2 if inc16 else 0)
    lines = 2 * ((prof_rows + 1) // 2) if inc16 and Gb == 64 else (prof_rows + rpl - 1) // rpl
    return (144 + nw * (4 * 64 + 2 * MAX_SEG + nseg_max * WIN)) * 4 + lines * row_dwords * 256


def max_waves(W):
    return 8 if W <= 24 else 4


def inc16_fits(W, Gb):
    if W > INC16_MAX_W:
        return False
    nw = 4
    while nw <= max_waves(W):
        if (LDS_PER_CU // lds_bytes(W, Gb, nw, True)) * nw >= 16:
            return True
        nw *= 2
    return False


def model_step(W, nseg):
    pen = 1.15 if W >= 64 else 1.08 if W >= 48 else 1.04 if W >= 32 else 1.022 if W >= 24 else 1.014 if W >= 22 else 1.0
    return (W + 0.3 + 0.535 * nseg) * pen


def model_inc16(W, Gb):
    return W <= INC16_MAX_W and ((Gb <= 16 and W <= 22) or (Gb == 32 and 11 <= W <= 19))


def model_choice(lb):
    best, best_cost = None, 0.0
    for W in VARIANTS:
        G = lanes(lb, W)
        if G > 64:
            continue
        cost = model_step(W, nseg_of(G)) * (0.94 if model_inc16(W, g_bucket(G)) else 1.0) / nseg_of(G)
        if best is None or cost < best_cost:
            best, best_cost = W, cost
    return best


class Table:
    """The record as the header holds it: 64-row points in the model's units, float32, four decimals."""

    def __init__(self, path=RECORD):
        rec = json.load(open(path))
        pts = [p for p in rec["points"] if p["rows"] == 64]
        k = float(np.median([p["step_ns"] / model_step(p["W"], p["nseg"]) for p in pts])) if pts else 1.0
        f32 = lambda x: float(np.float32(f"{x:.4f}"))
        same = {}                                             # two lengths may give one (W, cell, G): one point, their mean; the spread covers both
        for p in pts:
            same.setdefault((p["W"], p["cell"], p["G"]), []).append((p["step_ns"] / k, p["step_spread_ns"] / k))
        self.points = []
        for key, v in same.items():
            mean = sum(s for s, _ in v) / len(v)
            self.points.append(key + (f32(mean), f32(max(max(e for _, e in v), max(abs(s - mean) for s, _ in v)))))
        self.points.sort()
        self.pins = [(p["first"], p["last"]) for p in rec.get("pins", [])]
        self.hash = rec.get("kernel_source_hash")
        self._cell = {}

    def pinned(self, lb):
        return any(lo <= lb <= hi for lo, hi in self.pins)

    def rate_at(self, W, G, cell):
        """(step, spread) or None: linear in G between two measured lengths of one bucket; beyond them only while the segments
        per wave stay those of the nearest point."""
        lo = hi = None
        for p in self.points:
            if p[0] != W or p[1] != cell or g_bucket(p[2]) != g_bucket(G):
                continue
            if p[2] <= G and (lo is None or p[2] > lo[2]):
                lo = p
            if p[2] >= G and (hi is None or p[2] < hi[2]):
                hi = p
        if lo and hi:
            t = 0.0 if hi[2] == lo[2] else (G - lo[2]) / (hi[2] - lo[2])
            return lo[3] + t * (hi[3] - lo[3]), max(lo[4], hi[4])
        p = lo or hi
        if p is None or nseg_of(p[2]) != nseg_of(G):
            return None
        return p[3], p[4]

    def class_inc16(self, W, G):
        """The cell of launch class (W, bucket of G): the cheaper one of the table, summed over the lengths it holds both at, where the
        profile cell is compiled and a workgroup shape holds its profile; the model's where the record is silent or undecided."""
        Gb = g_bucket(G)
        if W > INC16_MAX_W or Gb > 32:
            return False
        if (W, Gb) not in self._cell:
            said = None
            if inc16_fits(W, Gb):
                prof = comp = err = 0.0
                n = 0
                for p in self.points:
                    if p[0] == W and p[1] == 1 and g_bucket(p[2]) == Gb:
                        for q in self.points:
                            if q[0] == W and q[1] == 0 and q[2] == p[2]:
                                prof += p[3]; comp += q[3]; err += p[4] + q[4]; n += 1
                if n and prof + err < comp:
                    said = True
                if n and comp + err < prof:
                    said = False
            self._cell[(W, Gb)] = model_inc16(W, Gb) if said is None else said
        return self._cell[(W, Gb)]

    def rate_of(self, W, lb):
        G = lanes(lb, W)
        if G > 64:
            return None
        r = self.rate_at(W, G, 1 if self.class_inc16(W, G) else 0)
        return None if r is None else (r[0] / nseg_of(G), r[1] / nseg_of(G))

    def choice(self, lb):
        """Argmin of the table under the hysteresis rule: the model's choice unless a variant the record prices is cheaper than it by
        more than the two points' spread; the cheapest of those."""
        best = model_choice(lb)
        if self.pinned(lb):
            return best
        base = self.rate_of(best, lb)
        if base is None:
            return best
        best_cost = base[0]
        for W in VARIANTS:
            r = self.rate_of(W, lb)
            if r is not None and r[0] + r[1] + base[1] < base[0] and r[0] < best_cost:
                best, best_cost = W, r[0]
        return best

    def remainder(self, lb, r, W0):
        """pc_nw_choose_remainder: the variant (columns per lane) for the last r rows of a bucket on W0, or None (they stay)."""
        G0 = lanes(lb, W0)
        if G0 > 64 or nseg_of(G0) <= 1 or r >= nseg_of(G0):
            return None
        margin = 0.7
        best, best_cost = None, margin * model_step(W0, nseg_of(G0))
        for W in VARIANTS:
            G = lanes(lb, W)
            if G > 64:
                continue
            cost = model_step(W, nseg_of(G)) * (-(-r // nseg_of(G)))
            if cost < best_cost:
                best, best_cost = W, cost
        stay = self.rate_at(W0, G0, 0)
        if self.pinned(lb) or stay is None:
            return best

        def tab(W):
            G = lanes(lb, W)
            got = None if G > 64 else self.rate_at(W, G, 0)
            if got is None:
                return None
            rounds = -(-r // nseg_of(G))
            return got[0] * rounds, got[1] * rounds
        cur, cur_e = margin * stay[0], margin * stay[1]
        if best is not None:
            got = tab(best)
            if got is None:
                return best
            if got[0] - got[1] > cur + cur_e:
                best = None
            else:
                cur, cur_e = got
        pick, pick_cost = best, cur
        for W in VARIANTS:
            got = None if W == W0 else tab(W)
            if got is not None and got[0] + got[1] + cur_e < cur and got[0] < pick_cost:
                pick, pick_cost = W, got[0]
        return pick

    def waves(self, W, G, cell_mode=0):
        """waves_for: cell_mode 0 = the class's own cell, 1 = compare, 2 = profile (percent-positives)"""
        inc16 = (W <= INC16_MAX_W and G <= 64) if cell_mode == 2 else (cell_mode == 0 and self.class_inc16(W, G))
        if not inc16:
            return 4
        nw = 4
        while nw <= max_waves(W):
            if (LDS_PER_CU // lds_bytes(W, g_bucket(G), nw, True)) * nw >= 16:
                return nw
            nw *= 2
        return max_waves(W)

    def launch_lds(self, W, lb, mode, ppos=False, compare_only=False):
        """launch_shape: (waves, profile cell?, LDS bytes) of a launch of this class whose longest column gene has lb residues;
        mode 0 = the class's workgroup, 1 = two waves, 2 = one wave"""
        G = min(64, max(1, lanes(lb, W)))
        cell_mode = 2 if ppos else 1 if (compare_only or mode == 2) else 0
        nw = 1 if mode == 2 else 2 if mode == 1 else self.waves(W, G, cell_mode)
        inc16 = (W <= INC16_MAX_W) if cell_mode == 2 else (cell_mode == 0 and self.class_inc16(W, G))
        return nw, inc16, lds_bytes(W, G, nw, inc16, cell_mode == 2)


def moved_lengths(table, top=MAX_LB):
    """Lengths at which the table's choice differs from the model's, and the lengths on both sides of each boundary of such a run."""
    moved = [lb for lb in range(1, top + 1) if table.choice(lb) != model_choice(lb)]
    edges = set()
    for lb in moved:
        if lb - 1 not in moved or lb + 1 not in moved or table.choice(lb) != table.choice(lb - 1) or table.choice(lb) != table.choice(lb + 1):
            edges |= {max(1, lb - 1), lb, min(top, lb + 1)}
    return moved, sorted(edges)
