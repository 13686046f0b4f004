// pc_nw_shape.hip -- K4's launch arithmetic: the variant, cell, remainder and percent-positives choosers with the readers of the rate
// table (pc_nw_rates.h), the launch classes and the cut of a bucket into tasks, and the shape of every launch (waves, LDS, rows per task,
// task mode, fuse key, strip form, scratch sizes).  Host only, no device code, no context: it reads its arguments, the table and the
// environment switches.  The kernels and their launchers are pc_nw_systolic.h and pc_nw.hip; what both sides share is pc_nw_geometry.h.
#include "pc_nw_geometry.h"
#include "pc_nw_rates.h"        // measured step costs the choosers read
#include "../../include/phamclust_hip.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

// columns-per-lane of the compiled systolic variants
static const int g_variant_w[] = {2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 24, 32, 48, 64};
static const int g_num_variants = (int)(sizeof(g_variant_w) / sizeof(int));

int pc_nw_num_variants() { return g_num_variants; }
int pc_nw_variant_w(int v) { return (v >= 0 && v < g_num_variants) ? g_variant_w[v] : 0; }
int pc_nw_variant_takes_any_byte(int v) { return v < 0 || v >= g_num_variants || g_variant_w[v] > PC_INC16_MAX_W; }   // 0: some class of this variant may run the profile cell

// PC_RATE_TABLE=0|1|2|3 (A/B): bit 0 the variant and remainder choosers read the table, bit 1 the cell rule does; default both
static int rate_table_use() { static const int m = getenv("PC_RATE_TABLE") ? atoi(getenv("PC_RATE_TABLE")) : 3; return m; }
static int inc16_forced() { static const int force = getenv("PC_INC16") ? atoi(getenv("PC_INC16")) : -1; return force; }   // tuning: 0 = never, 1 = wherever compiled (up to 32 lanes per segment), 2 = wherever a workgroup shape fits (64 lanes included: tools/class_rates.py)
static bool strip_enabled() { static const bool off = getenv("PC_STRIP") && !atoi(getenv("PC_STRIP")); return !off; }

// LDS of one workgroup: score table, the waves' private regions, the profile of a column gene spread over G lanes
static size_t systolic_lds_bytes(int W, int G, int nw, bool inc16, bool any_bucket = false) {
    const int Gb = pc_nw_g_bucket(G), rpl = 64 / Gb;                      // profile rows per 64-dword line (see the kernel)
    const int nseg_max = pc_nw_segs_of((Gb == 8 || any_bucket) ? 1 : Gb / 2 + 1);   // the bucket's fewest lanes per segment (any_bucket: the launch's column genes may be shorter than its bucket)
    const size_t lines = (inc16 && Gb == 64) ? (size_t)2 * ((pc_prof_rows(inc16) + 1) / 2)       // two half tables of 2 rows per line
                                             : (size_t)((pc_prof_rows(inc16) + rpl - 1) / rpl);
    return (size_t)(PC_WG_HEADER_DWORDS + nw * pc_wave_lds_dwords(nseg_max)) * 4 + lines * pc_prof_row_dwords(W, inc16) * 256;
}
// Waves per workgroup of a class that runs the profile cell: the fewest (4, 8; at most what the variant's registers allow) that put
// 16 waves on a CU given the LDS the class's largest profile takes; 0 if none does
static int inc16_waves(int W, int Gb) {
    for (int nw = PC_MIN_WAVES; nw <= pc_max_waves(W); nw *= 2)
        if ((int)((size_t)160 * 1024 / systolic_lds_bytes(W, Gb, nw, true)) * nw >= 16) return nw;
    return 0;
}
// Does a workgroup shape hold the profile cell's profile of this launch class with 16 waves on a CU?
static bool inc16_fits(int W, int Gb) { return W <= PC_INC16_MAX_W && inc16_waves(W, Gb) != 0; }
static bool model_inc16(int W, int Gb) {                                            // the r02 rule (see class_inc16)
    if (W > PC_INC16_MAX_W || Gb > 32) return false;
    if (inc16_forced() >= 0) return inc16_forced() != 0;
    return (Gb <= 16 && W <= 22) || (Gb == 32 && W >= 11 && W <= 19);
}
// Which cell a launch class runs: the cheaper one of the rate table (pc_nw_rates.h) where it holds both, else the r02 rule
// (measured per class with the launches serialised, profiles/r02/experiments/l_class_times.txt):
// the 16-bit increment profile wins 5-7 % where four workgroups still fit a CU beside it (segments of up to 16 lanes)
// and 3-5 % with 8-wave workgroups on segments of up to 32 lanes for W = 11..19 (W <= 9: -15..-40 %, short strips; W = 20: nothing; W = 24: -6 % in
// either bucket, its profile needs 8-wave groups even at 16 lanes); with
// one segment per wave (up to 64 lanes) the profile of a long gene leaves room for a single 16-wave workgroup per CU
// and loses 5-10 %.  Elsewhere the residue compare.
static bool class_inc16(int W, int G) {
    const int force = inc16_forced();
    if (W > PC_INC16_MAX_W) return false;
    const int Gb = pc_nw_g_bucket(G);
    if (force == 2) return inc16_fits(W, Gb);
    if (Gb > 32) return false;                                                        // (measured: no room for enough waves; only percent-positives launches run the profile cell there)
    if (force >= 0) return force != 0;
    // The cheaper cell of the rate table for this launch class (W, lanes-per-segment bucket), summed over the lengths at which the
    // record holds both -- where the profile cell is compiled and a workgroup shape holds its profile (inc16_fits); the r02 rule
    // stands where the record is silent or the two differ by less than their spread
    static const std::vector<int8_t> by_table = [] {
        std::vector<int8_t> t((PC_INC16_MAX_W + 1) * 4, -1);
        for (int w = 1; w <= PC_INC16_MAX_W; ++w)
            for (int b = 0; b < 3; ++b) {
                const int gb = 8 << b;
                if (!inc16_fits(w, gb) || !(rate_table_use() & 2)) continue;
                double prof = 0, comp = 0, err = 0; int n = 0;
                for (int i = 0; i < pc_nw_n_rates; ++i) {
                    const PcRatePoint& p = pc_nw_rates[i];
                    if (p.W != w || p.cell != 1 || pc_nw_g_bucket(p.G) != gb) continue;
                    for (int k = 0; k < pc_nw_n_rates; ++k) {
                        const PcRatePoint& q = pc_nw_rates[k];
                        if (q.W == w && q.cell == 0 && q.G == p.G) { prof += p.step; comp += q.step; err += p.spread + q.spread; ++n; }
                    }
                }
                if (n && prof + err < comp) t[w * 4 + b] = 1;
                if (n && comp + err < prof) t[w * 4 + b] = 0;
            }
        return t;
    }();
    const int said = by_table[W * 4 + pc_nw_g_index(G)];
    return said >= 0 ? said != 0 : model_inc16(W, Gb);
}
// cell_mode: 0 = the class's own choice, 1 = compare cell ("any byte" classes), 2 = profile cell (percent-positives runs)
static bool mode_inc16(int W, int G, int cell_mode) {
    if (cell_mode == 2) return W <= PC_INC16_MAX_W && G <= 64;
    return cell_mode == 0 && class_inc16(W, G);
}
// Waves per workgroup: the compare cell's profile is small, four do; the profile cell's as inc16_waves finds, the most allowed if none fits
static int waves_for(int W, int G, int cell_mode) {
    if (!mode_inc16(W, G, cell_mode)) return PC_MIN_WAVES;
    const int nw = inc16_waves(W, pc_nw_g_bucket(G));
    return nw ? nw : pc_max_waves(W);
}
int pc_nw_class_waves(int variant, int lb, int compare_only) {
    if (variant < 0 || variant >= g_num_variants || lb <= 0) return PC_MIN_WAVES;
    const int W = g_variant_w[variant];
    return waves_for(W, pc_nw_lanes(lb, W), compare_only != 0 ? 1 : 0);
}

// Variant for a column gene of lb residues: the model below, corrected by the measured rate table (pc_nw_rates.h) where the record prices
// both the model's choice and a cheaper variant -- see choose_variant_uncached.
// The model.  Time per row step ~ (W + c0 + c1 nseg) cell-equivalents (x 1.014 at
// W = 22, x 1.022 at W = 24: three waves per SIMD), during which a wave retires nseg rows of lb cells; c1 = 0.535
// from a least-squares fit to measured kernel-only GCUPS of every variant over L = 60..1200
// (profiles/r01/experiments/l_variant_gcups.txt), c0 = 0.3 after the step prologue shrank to ~12 instructions (end-to-end
// sweep: the fill time is flat within 1 % over c0 = 0.3..1.0).  The nseg term stands for what short sequences pay
// per alignment and per task (virtual row, pipeline fill, profile build).  Minimise cost per retired row over the
// variants whose 64*W columns cover lb.
// Column genes beyond the widest variant's 4,096 columns run strip-mined (k_nw_strip): ceil(lb / 64 W) passes of a wide variant,
// a pass costing a row step of that variant per row whatever its width -- the fewest step-instructions win (W = 32 / 48 / 64:
// 2,048 / 3,072 / 4,096 columns per pass; penalties as below).  PC_STRIP=0 sends them to the general kernel as r01-r03 did.

// Does a launch of this class run on k_nw_strip (and need the scratch slab)?  Column genes beyond the variant's 64 x W columns
// always; and the one- / two-row tasks of the wide variants' ordinary classes, which narrow passes serve better (see PC_STRIP_W_*).
int pc_nw_launch_is_strip(int variant, int max_lb, int wave_mode, int ppos) {
    if (variant < 0 || variant >= g_num_variants) return 0;
    const int W = g_variant_w[variant];
    if (max_lb > 64 * W) return 1;
    return (!ppos && W >= 32 && wave_mode != PC_MODE_CLASS && strip_enabled()) ? 1 : 0;
}
int pc_nw_strip_passes(int lb, int variant) {
    if (variant < 0 || variant >= g_num_variants || lb <= 0) return 0;
    return pc_nw_lanes(lb, 64 * g_variant_w[variant]);
}
static int choose_strip_variant(int lb) {
    if (!strip_enabled()) return -1;
    int best = -1; double best_cost = 0;
    for (int v = 0; v < g_num_variants; ++v) {
        const int W = g_variant_w[v];
        if (W < 32) continue;
        const double pen = W >= 64 ? 1.15 : W >= 48 ? 1.08 : 1.04;
        const double cost = (double)pc_nw_strip_passes(lb, v) * (W + 1.0) * pen;
        if (best < 0 || cost < best_cost) { best = v; best_cost = cost; }
    }
    return best;
}
// ---- the model (r01-r04): what a point the rate table does not cover is priced by, and "today's choice" that a tabulated
// point has to beat by more than its spread.  Time per row step ~ (W + c0 + c1 nseg) cell-equivalents, x the occupancy penalty of
// the wide tiers, x 0.94 where the class runs the profile cell.
static double model_step(int W, int nseg) {
    const double pen = W >= 64 ? 1.15 : W >= 48 ? 1.08 : W >= 32 ? 1.04 : W >= 24 ? 1.022 : (W >= 22 ? 1.014 : 1.0);
    return (W + 0.3 + 0.535 * nseg) * pen;
}
static int model_choose_variant(int lb, int cap = 0) {                   // cap > 0 (PC_CHOOSE_MAX_W): no variant wider, and the step as the compare cell's
    int best = -1; double best_cost = 0;
    for (int v = 0; v < g_num_variants; ++v) {
        const int W = g_variant_w[v], G = pc_nw_lanes(lb, W);
        if (G > 64 || (cap > 0 && W > cap)) continue;
        const int nseg = pc_nw_segs_of(G);
        const bool inc16 = cap <= 0 && model_inc16(W, pc_nw_g_bucket(G));
        const double cost = model_step(W, nseg) * (inc16 ? 0.94 : 1.0) / nseg;
        if (best < 0 || cost < best_cost) { best = v; best_cost = cost; }
    }
    return best;
}

// ---- the rate table (pc_nw_rates.h): step cost of (W, G lanes per segment, cell) where the record holds it.  Between two measured
// lengths of one lanes-per-segment bucket: linear in G; beyond them only as far as the segments per wave stay those of the
// nearest point (a wave's step does not depend on how many of a segment's lanes work).
static bool rate_at(int W, int G, int cell, double& step, double& spread) {
    const int Gb = pc_nw_g_bucket(G);
    const PcRatePoint *lo = nullptr, *hi = nullptr;
    for (int i = 0; i < pc_nw_n_rates; ++i) {
        const PcRatePoint& p = pc_nw_rates[i];
        if (p.W != W || p.cell != cell || pc_nw_g_bucket(p.G) != Gb) continue;
        if (p.G <= G && (!lo || p.G > lo->G)) lo = &p;
        if (p.G >= G && (!hi || p.G < hi->G)) hi = &p;
    }
    if (lo && hi) {
        const double t = hi->G == lo->G ? 0.0 : (double)(G - lo->G) / (hi->G - lo->G);
        step = lo->step + t * (hi->step - lo->step);
        spread = std::max(lo->spread, hi->spread);
        return true;
    }
    const PcRatePoint* p = lo ? lo : hi;
    if (!p || pc_nw_segs_of(p->G) != pc_nw_segs_of(G)) return false;
    step = p->step; spread = p->spread;
    return true;
}
static bool rate_pinned(int lb) {
    if (!(rate_table_use() & 1)) return true;
    for (int i = 0; i < pc_nw_n_rate_pins; ++i) if (lb >= pc_nw_rate_pins[i][0] && lb <= pc_nw_rate_pins[i][1]) return true;
    return false;
}
// Cost per alignment row of a column gene of lb residues on variant v in the cell its class runs, from the table
static bool rate_of(int v, int lb, double& cost, double& spread) {
    const int W = g_variant_w[v], G = pc_nw_lanes(lb, W);
    if (G > 64) return false;
    double s, e;
    if (!rate_at(W, G, class_inc16(W, G) ? 1 : 0, s, e)) return false;
    cost = s / pc_nw_segs_of(G); spread = e / pc_nw_segs_of(G);
    return true;
}
// PC_CHOOSE_MAX_W=w (A/B): no variant wider than w for a column gene that a narrower one holds
static int choose_max_w() { static const int w = getenv("PC_CHOOSE_MAX_W") ? atoi(getenv("PC_CHOOSE_MAX_W")) : 0; return w; }
static int choose_variant_uncached(int lb) {
    int best = model_choose_variant(lb);
    const int cap = choose_max_w();
    if (cap > 0 && best >= 0 && g_variant_w[best] > cap && lb <= 64 * cap) return model_choose_variant(lb, cap);
    // the table's say: a variant takes the place of the model's choice only if the record prices both and it is cheaper by more
    // than the two points' spread (noise stays out of the policy); the cheapest of those that are
    double c0, e0;
    if (best < 0 || rate_pinned(lb) || !rate_of(best, lb, c0, e0)) return best;
    double best_cost = c0;
    for (int v = 0; v < g_num_variants; ++v) {
        double c, e;
        if (!rate_of(v, lb, c, e)) continue;
        if (c + e + e0 < c0 && c < best_cost) { best = v; best_cost = c; }
    }
    return best;
}
int pc_nw_choose_variant(int lb) {
    if (lb <= 0) return -1;
    if (lb > 64 * PC_MAX_W) return choose_strip_variant(lb);
    static const std::vector<int8_t> memo = [] {                         // (a fill asks once per distinct length, pc_align_pairs once per pair)
        std::vector<int8_t> m(64 * PC_MAX_W + 1, -1);
        for (int l = 1; l <= 64 * PC_MAX_W; ++l) m[l] = (int8_t)choose_variant_uncached(l);
        return m;
    }();
    return memo[lb];
}

// A bucket whose row count is not a multiple of its variant's nseg leaves r = n mod nseg rows for a last wave round in
// which only r of the nseg segments work.  Those r rows can go to a variant with fewer, longer segments instead:
// returns that variant, or -1 when staying is as cheap (the cost of a wave round is the step cost of the variant;
// 30 % margin for the extra workgroup).  Step costs: the model's; the table's (compare cell: such a task runs in a one-wave
// workgroup) where it prices the staying round and the candidate both, under the same rule as the variant chooser -- the
// model's answer stands unless the record contradicts it by more than the spread.
int pc_nw_choose_remainder(int lb, int r, int main_variant) {
    static const bool off = getenv("PC_REMAINDER") && !strcmp(getenv("PC_REMAINDER"), "0");
    if (off || lb <= 0 || r <= 0 || main_variant < 0 || main_variant >= g_num_variants) return -1;
    const int W0 = g_variant_w[main_variant], G0 = pc_nw_lanes(lb, W0);
    const int nseg0 = pc_nw_segs_of(G0);
    if (nseg0 <= 1 || r >= nseg0) return -1;                              // (a strip-mined gene: one row per wave)
    constexpr double margin = 0.7;
    int best = -1; double best_cost = margin * model_step(W0, nseg0);
    for (int v = 0; v < g_num_variants; ++v) {
        const int W = g_variant_w[v], G = pc_nw_lanes(lb, W);
        if (G > 64) continue;
        const int nseg = pc_nw_segs_of(G);
        const double cost = model_step(W, nseg) * ((r + nseg - 1) / nseg);
        if (cost < best_cost) { best = v; best_cost = cost; }
    }
    double s0, e0;
    if (rate_pinned(lb) || !rate_at(W0, G0, 0, s0, e0)) return best;
    auto tab = [&](int v, double& c, double& e) {
        const int W = g_variant_w[v], G = pc_nw_lanes(lb, W);
        if (G > 64 || !rate_at(W, G, 0, c, e)) return false;
        const int rounds = (r + pc_nw_segs_of(G) - 1) / pc_nw_segs_of(G);
        c *= rounds; e *= rounds;
        return true;
    };
    double cur = margin * s0, cur_e = margin * e0;                        // today's choice in the table's units: stay ...
    if (best >= 0) {                                                      // ... or the model's move, unless the record says it loses
        double c, e;
        if (!tab(best, c, e)) return best;
        if (c - e > cur + cur_e) best = -1; else { cur = c; cur_e = e; }
    }
    int pick = best; double pick_cost = cur;
    for (int v = 0; v < g_num_variants; ++v) {
        double c, e;
        if (v == main_variant || !tab(v, c, e)) continue;
        if (c + e + cur_e < cur && c < pick_cost) { pick = v; pick_cost = c; }
    }
    return pick;
}

// Percent-positives (aai with ppos=True) needs the profile cell -- "positive" is a property of (row residue, column residue),
// i.e. a table entry, not a residue compare: systolic where that cell can run, the general kernel elsewhere
#define PC_STRIP_PPOS_MAX_LB 8191                     // the profile cell's statistics are 13-bit fields (PC_INC16_K)
int pc_nw_ppos_systolic(int variant, int max_lb) {
    if (variant < 0 || variant >= g_num_variants || max_lb <= 0) return 0;
    const int W = g_variant_w[variant];
    if (max_lb > 64 * W) return (W == PC_INC16_MAX_W && strip_enabled() && max_lb <= PC_STRIP_PPOS_MAX_LB) ? 1 : 0;   // strip-mined passes of W = 24
    return mode_inc16(W, pc_nw_lanes(max_lb, W), 2) ? 1 : 0;
}
// ... and for a class whose own variant cannot (the wide ones, W >= 32, have no profile cell): the widest variant that has
// one, if it can take the class's longest column gene (tasks do not depend on the variant that runs them); -1: none,
// i.e. column genes over 64 x 24 = 1,536 residues stay on the general kernel
int pc_nw_ppos_variant(int max_lb) {
    for (int v = g_num_variants - 1; v >= 0; --v) if (pc_nw_ppos_systolic(v, max_lb)) return v;
    return -1;
}

// Rows (alignments) per workgroup task for a column gene of lb residues.  A task's 4*nseg row streams each walk
// rows/(4*nseg) rows of ~lb residues, one residue per step, a step costing ~(W+1) cell slots: a fixed 208 rows makes
// the tasks of long genes (one segment per wave) run a hundred times longer than those of short ones, and the
// longest task bounds the fill from below once the work is split over ranks (or N is small).  So a stream is capped
// at ~PC_TASK_BUDGET cell slots (never below one row per stream, never above PC_TASK_ROWS rows per task).
static int task_budget() { static const int b = getenv("PC_TASK_BUDGET") ? atoi(getenv("PC_TASK_BUDGET")) : 0; return b > 0 ? b : PC_TASK_BUDGET; }
int pc_nw_task_rows(int lb, int variant, int compare_only) {
    if (variant < 0 || variant >= g_num_variants || lb <= 0) return 64;       // general kernel: one pass of 64 rows
    const int W = g_variant_w[variant];
    if (pc_nw_lanes(lb, W) > 64) return PC_STRIP_WAVES;                       // strip-mined: one row per wave, pass after pass
    const int nseg = pc_nw_segs(lb, W);
    const int64_t steps = task_budget() / (W + 1);
    int64_t per_stream = steps / (lb + 1); if (per_stream < 1) per_stream = 1;
    const int nw = pc_nw_class_waves(variant, lb, compare_only);
    int64_t rows = per_stream * nw * nseg;
    const int64_t wave_cap = (int64_t)nw * (64 / nseg) * nseg;           // a wave keeps at most 64 rows (ceil(R / (nw nseg)) nseg of the task's R)
    if (rows > wave_cap) rows = wave_cap;
    return (int)(rows > PC_TASK_ROWS ? PC_TASK_ROWS : rows);
}

// Launch mode of a task of `rows` rows against a column gene of lb residues on variant W (host mirror of pc_task_mode in
// pc_plan.hip).  A workgroup's waves beyond ceil(rows / nseg) find no row and leave at once, but the LDS sized for all of them
// stays taken until the last wave is done -- with the profile cell's 20-28 KB that is five workgroups per CU with ONE live wave
// each.  Measured on uniform 207-residue genes (tools/bucket_size_bench.py, GCUPS at 1 / 2 / 4 / 8 rows per column gene):
// 4-wave profile-cell workgroups 452 / 894 / 1,726 / 2,344; one wave + compare cell 659 / 1,297 / 2,567 / 2,649; two waves
// 491 / 962 / 1,907 / 2,550 (compare cell 2,681); from 16 rows the 4-wave groups win (2,956 against 2,732-2,853).
int pc_nw_task_mode(int lb, int rows, int variant) {
    static const int off = getenv("PC_SMALL_MODES") ? !atoi(getenv("PC_SMALL_MODES")) : 0;       // PC_SMALL_MODES=0: every task in its class's own workgroup shape
    if (off || variant < 0 || variant >= g_num_variants || lb <= 0) return PC_MODE_CLASS;
    return pc_nw_mode_of(rows, pc_nw_segs(lb, g_variant_w[variant]));
}
int pc_nw_small_modes_enabled() { return pc_nw_task_mode(64, 1, 0) != PC_MODE_CLASS; }

// the launch classes (numbering: pc_common.h) and the cut of a bucket into tasks
int pc_num_classes() { return g_num_variants * 8 + PC_STRIP_CLASSES + 1; }
int pc_class_of(int lb, int variant, bool any_byte) {
    const int nvar = g_num_variants;
    if (variant < 0) return nvar * 8 + PC_STRIP_CLASSES;
    const int W = pc_nw_variant_w(variant);
    if (lb > 64 * W) return nvar * 8 + std::max(0, variant - (nvar - PC_STRIP_CLASSES));       // strip-mined (the chooser only picks a wide variant for these)
    return variant * 4 + pc_nw_g_index(pc_nw_lanes(lb, W)) + (any_byte && !pc_nw_variant_takes_any_byte(variant) ? nvar * 4 : 0);
}
int pc_class_variant(int cls) {
    const int nvar = g_num_variants;
    if (cls >= nvar * 8 + PC_STRIP_CLASSES) return -1;
    if (cls >= nvar * 8) return nvar - PC_STRIP_CLASSES + (cls - nvar * 8);
    return (cls % (nvar * 4)) / 4;
}
int pc_class_compare_only(int cls) { return cls >= g_num_variants * 4 && cls < g_num_variants * 8; }
PcBucketCut pc_bucket_cut(int lb, int64_t rows, int base, bool any_byte, bool move_remainder) {
    const int v = pc_class_variant(base);
    PcBucketCut cut{pc_nw_task_rows(lb, v, pc_class_compare_only(base)), rows, -1};
    if (move_remainder && v >= 0) {
        const int nseg = pc_nw_segs(lb, pc_nw_variant_w(v));
        const int r = nseg > 1 ? (int)(rows % nseg) : 0;
        const int vr = r ? pc_nw_choose_remainder(lb, r, v) : -1;
        if (vr >= 0) { cut.n_main = rows - r; cut.rem_base = pc_class_of(lb, vr, any_byte); }
    }
    return cut;
}
int pc_task_launch_class(int lb, int rows, int base, bool modes) {
    return base * PC_WAVE_MODES + (modes ? pc_nw_task_mode(lb, rows, pc_class_variant(base)) : (int)PC_MODE_CLASS);
}

// Workgroup shape of a strip-mined launch: one row per wave (4 / 2 / 1 waves by the tasks' rows), or -- `pipe` -- the passes of one
// alignment dealt over 8 or 4 waves, a workgroup per row (k_nw_strip's PIPE form).  A lone wave retires a 6,600 x 6,600 alignment in
// T1 = 47 ms; eight waves in T1 / 6.4, four in T1 / 3.2, at 1 resp. 3 workgroups per CU instead of 11 one-wave ones.  So: the
// pipeline while the launch's rows fit the chip in a round or two of it (the alignment's latency is then the launch's
// duration, and on small fills the fill's), one row per wave beyond (more rows in flight, same instructions).
// PC_PIPE=0: never; PC_PIPE=n: always, n waves.
static void strip_workgroup(int wave_mode, int ntasks, int ppos, int n_cu, PcLaunchShape& sh) {
    const char* env = getenv("PC_PIPE");                                  // (read per launch: the tests switch it between fills)
    const int forced = env && *env ? atoi(env) : -1;
    const int cu = n_cu > 0 ? n_cu : 256;
    const int nw = wave_mode == PC_MODE_ONE_WAVE ? 1 : wave_mode == PC_MODE_TWO_WAVES ? 2 : PC_STRIP_WAVES;
    const long long rows = (long long)ntasks * nw;                       // (at most: a task of the 4- / 2- / 1-wave shape holds up to that many rows)
    sh.strip = true; sh.pipe = true;
    if (ppos || forced == 0) { sh.pipe = false; sh.nw = nw; }
    else if (forced > 0) sh.nw = forced < PC_PIPE_WAVES_MAX ? forced : PC_PIPE_WAVES_MAX;
    else if (rows <= cu) sh.nw = PC_PIPE_WAVES_MAX;
    else if (rows <= (wave_mode == PC_MODE_CLASS ? 3 : 6) * cu) sh.nw = 4;
    else { sh.pipe = false; sh.nw = nw; }
    sh.per_cu = sh.pipe ? (sh.nw > 4 ? 1 : 3) : (sh.nw == 1 ? 12 : sh.nw == 2 ? 8 : 3);
}
// The launch's shape, whichever kernel runs it (`variant` is one of the compiled ones).  A systolic launch of one class: which cell
// it runs, waves per workgroup, dynamic LDS.  Strip-mined: the width is the launch's choice, not the class's -- few tasks: the passes
// of each alignment over the waves of a workgroup, narrow passes whatever the class's width; tasks of one row / two rows: narrow
// passes in one- / two-wave workgroups; percent-positives: the profile cell's widest variant.
int pc_nw_launch_shape(int variant, int max_lb, int ppos, int compare_only, int wave_mode, int ntasks, int n_cu, PcLaunchShape& sh) {
    const int W = g_variant_w[variant];
    if (!pc_nw_launch_is_strip(variant, max_lb, wave_mode, ppos)) {
        const int Gmax = pc_nw_launch_lanes(max_lb, W), cell_mode = ppos ? 2 : ((compare_only != 0 || wave_mode == PC_MODE_ONE_WAVE) ? 1 : 0);
        // small tasks (pc_nw_task_mode): all their rows fit one or two waves, and a workgroup sized for them leaves its LDS to others
        sh = PcLaunchShape{W, wave_mode == PC_MODE_ONE_WAVE ? 1 : wave_mode == PC_MODE_TWO_WAVES ? 2 : waves_for(W, Gmax, cell_mode),
                           W <= PC_INC16_MAX_W && mode_inc16(W, Gmax, cell_mode), false, false, 0, 0};
        if (ppos && !sh.inc16) { pc_set_error("k_nw_systolic<%d>: percent-positives needs the profile cell (W <= %d)", W, PC_INC16_MAX_W); return PC_ERR_ARG; }
        sh.lds = systolic_lds_bytes(W, Gmax, sh.nw, sh.inc16, cell_mode == 2);
        return PC_OK;
    }
    sh = PcLaunchShape{};
    strip_workgroup(wave_mode, ntasks, ppos, n_cu, sh);
    sh.inc16 = ppos && W == PC_INC16_MAX_W;
    sh.W = sh.pipe ? PC_STRIP_W_ONE_ROW : sh.inc16 ? W : ppos ? 0 : sh.nw == 1 ? PC_STRIP_W_ONE_ROW : sh.nw == 2 ? PC_STRIP_W_TWO_ROWS : W >= 32 ? W : 0;
    if (!sh.W) { pc_set_error("pc_launch_nw: variant %d (w = %d) cannot take %d columns", variant, W, max_lb); return PC_ERR_ARG; }
    const size_t lines = sh.inc16 ? (size_t)2 * ((pc_prof_rows(true) + 1) / 2) : (size_t)pc_prof_rows(false);
    sh.lds = (size_t)(PC_WG_HEADER_DWORDS + sh.nw * pc_strip_wave_lds_dwords()) * 4
           + (sh.pipe ? (size_t)sh.nw : (size_t)1) * lines * pc_prof_row_dwords(sh.W, sh.inc16) * 256;   // pipe: a profile per wave
    return PC_OK;
}
// Launch classes that may share one k_nw_systolic_tier launch get the same key (>= 0): same register tier, same cell, same waves
// per workgroup -- and, for the one- and two-wave modes, the same lanes-per-segment bucket: their workgroups are small, so the
// LDS of the widest profile in the launch would cost the narrow ones their occupancy (a 4- or 8-wave workgroup spends at most
// ~9 KB of LDS per wave on the largest profile of its tier, within what the tier's registers let a CU hold anyway).
// -1: launched on its own (wide variants, strip-mined passes, the general kernel).
int pc_nw_fuse_key(int variant, int max_lb, int ppos, int compare_only, int wave_mode) {
    static const bool off = getenv("PC_FUSE") && !atoi(getenv("PC_FUSE"));
    if (variant < 0 || variant >= g_num_variants || max_lb > 64 * g_variant_w[variant]) return -1;
    const int tier = pc_tier_of(g_variant_w[variant]);
    if (tier < 0) return -1;
    PcLaunchShape sh;
    if (pc_nw_launch_shape(variant, max_lb, ppos, compare_only, wave_mode, 0, 0, sh) != PC_OK) return -1;      // (never strip-mined: a tier's variant within its columns)
    const int bucket = pc_nw_g_index(pc_nw_launch_lanes(max_lb, sh.W));
    const int key = (((tier * 2 + (sh.inc16 ? 1 : 0)) * 16 + sh.nw) * 8 + (wave_mode == PC_MODE_CLASS ? 0 : bucket + 1));
    // PC_FUSE=0 (A/B): every launch class its own launch, so a key per (variant, cell, mode, lanes-per-segment bucket) -- what tells the
    // launch classes apart.  (The key was once mixed from the shared key and max_lb % 4096: two classes of different workgroup size
    // could collide and were refused as one group.)
    return off ? 1000000 + ((variant * 2 + (compare_only ? 1 : 0)) * PC_WAVE_MODES + wave_mode) * 4 + bucket : key;
}

// Scratch of a strip-mined launch: one boundary line per wave of every resident workgroup (pc_strip_block_bytes)
size_t pc_nw_strip_scratch_bytes(int max_row_len, int n_cu) {
    const size_t per = pc_strip_block_bytes(max_row_len, PC_STRIP_WAVES);     // (sized for 4-wave workgroups, two per CU; one-wave launches
    size_t blocks = (size_t)3 * (n_cu > 0 ? n_cu : 256);                      //  then get 12 workgroups per CU out of the same slab)
    const size_t budget = (size_t)1 << 30;
    if (blocks * per > budget) blocks = std::max<size_t>(budget / per, 8);
    return blocks * per;
}
// ... and of ONE strip-mined launch of `ntasks` tasks that gets a region of its own (run_align_classes: such launches then run side by
// side, on their own streams, instead of one after the other on the one slab): a line per wave of as many workgroups as the
// chip holds of that shape, or as the launch has tasks
size_t pc_nw_strip_launch_bytes(int wave_mode, int ntasks, int max_row_len, int n_cu, int ppos) {
    PcLaunchShape sh; strip_workgroup(wave_mode, ntasks, ppos, n_cu, sh);
    size_t blocks = (size_t)sh.per_cu * (size_t)(n_cu > 0 ? n_cu : 256);
    const size_t units = (size_t)(ntasks > 0 ? ntasks : 1) * (sh.pipe ? PC_STRIP_WAVES : 1);       // (pipelined: a workgroup per row)
    if (blocks > units) blocks = units;
    return blocks * pc_strip_block_bytes(max_row_len, sh.nw);
}
size_t pc_nw_fallback_scratch_bytes(int max_lb) {
    const size_t per_block = (size_t)64 * (size_t)max_lb * sizeof(int4), budget = (size_t)2 << 30;
    return std::min<size_t>(std::max<size_t>(budget / (per_block ? per_block : 1), 32), 1024) * per_block;
}
