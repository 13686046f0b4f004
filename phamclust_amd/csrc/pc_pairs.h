// pc_pairs.h -- what the genome-pair kernel units share (pc_set_popc, pc_sparse, pc_sparse_col, pc_walk, pc_util) and what the host
// arithmetic of their launch shapes (pc_set_shape.hip) reads of them: the exact round(x, 6) and the epilogues built on it, the output
// index, the XCD-aware tile order, and the tile constants of the families.  Internal; everything here is static or inline.
//
// Reference semantics restated here (metrics.py of the reference):
//   metrics.py:45-48, 75, 104-110   the gcs / jc / pocp closed forms on two small integers (pc_set_value)
//   round(x, 6)                     CPython double_round: exact half-even on the binary value (pc_round6)
#pragma once
#include "pc_common.h"
#include <type_traits>
#include "../../include/phamclust_hip.h"

#define TS 32          // tile edge (genomes): k_sparse_tile's and the walkers' tiles

// ---------------------------------------------------------------------------------
// round(x, 6) exactly as CPython: decimal(x) correctly rounded half-even to 6 places,
// then the nearest double.  x in [0, 2^20).  x*1e6 = M * 15625 * 2^(e+6) exactly.
// ---------------------------------------------------------------------------------
// (one out-of-line copy per unit that finishes values: __noinline__ on purpose, see pc_round6)
static __device__ __noinline__ double pc_round6_exact(double x) {
    if (!(x > 0.0)) return 0.0;
    unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    int ex = (int)((bits >> 52) & 0x7ff);
    unsigned long long M = bits & ((1ULL << 52) - 1);
    int e;
    if (ex == 0) e = -1074; else { M |= 1ULL << 52; e = ex - 1075; }
    unsigned long long lo = M * 15625ULL, hi = __umul64hi(M, 15625ULL);   // P = hi:lo < 2^67
    int sh = -(e + 6);
    unsigned long long ip;
    if (sh <= 0) {
        ip = lo << (-sh);                                  // x >= 2^47: out of the documented domain, kept monotone
    } else if (sh >= 68) {
        ip = 0;                                            // x*1e6 < 0.5
    } else if (sh < 64) {
        ip = (sh == 0 ? lo : (lo >> sh)) | (hi << (64 - sh));
        unsigned long long frac = lo & ((1ULL << sh) - 1), half = 1ULL << (sh - 1);
        if (frac > half || (frac == half && (ip & 1))) ++ip;
    } else {
        int s2 = sh - 64;                                  // 0..3
        ip = hi >> s2;
        unsigned long long frac_hi = hi & ((1ULL << s2) - 1), frac_lo = lo;
        unsigned long long half_hi = s2 ? (1ULL << (s2 - 1)) : 0, half_lo = s2 ? 0 : (1ULL << 63);
        bool gt = frac_hi > half_hi || (frac_hi == half_hi && frac_lo > half_lo);
        bool eq = frac_hi == half_hi && frac_lo == half_lo;
        if (gt || (eq && (ip & 1))) ++ip;
    }
    return (double)ip / 1000000.0;
}

// The same value, usually in a dozen instructions.  y = fl(x * 1e6) is within 2^-33 of the exact product for x < 2, so
// when y is not within 2^-30 of a half-integer the exact product rounds (half-even or not: it is no tie) to rint(y), and the
// result is that integer divided by 1e6 -- the very division the exact routine ends with.  Only values that close to a
// decimal tie (two in a million) take the 128-bit integer route.  Every metric's epilogue runs this once or twice per genome
// pair; with the exact routine alone it was most of the sparse pocp / af kernel's time.
// k / 1e6 for an integer k in [0, 2^22], correctly rounded, in three instructions instead of the ~12 of a full fp64 division:
// q0 = k * RN(1e-6) is within an ulp of the quotient, r = k - q0 * 1e6 is exact in one fma, and q0 + r * RN(1e-6) rounds to the
// correctly rounded quotient (Markstein's final step: the divisor is a constant whose reciprocal is correctly rounded).  Held to
// `k / 1000000.0` for EVERY k of that range on the host (tests/test_oracle.py::test_markstein_division_by_a_million, plain C
// arithmetic) and on the device (tests/test_gpu_parity.py::test_round6_every_millionth: round6 of every k / 1e6 is itself).
__device__ __forceinline__ double pc_div_million(double k) {
    const double R = 1.0 / 1000000.0;
    const double q0 = k * R;
    const double r = __builtin_fma(-q0, 1000000.0, k);
    return __builtin_fma(r, R, q0);
}

__device__ __forceinline__ double pc_round6(double x) {
    if (!(x > 0.0)) return 0.0;
    if (x < 2.0) {
        const double y = x * 1.0e6;
        const double k = __builtin_rint(y);
        if (__builtin_fabs(y - k) <= 0.5 - 0x1p-30) return pc_div_million(k);
    }
    return pc_round6_exact(x);
}

__device__ __forceinline__ double pc_finish(double sim, int as_distance) {
    return as_distance ? pc_round6(1.0 - sim) : pc_round6(sim);
}

__device__ __forceinline__ int64_t pc_out_index(const PcDev& d, const PcShard& sh, int s, int t, int k, int condensed) {
    if (condensed) return (int64_t)s * d.N - (int64_t)s * (s + 1) / 2 + (t - s - 1);
    return sh.lbase[k] + s;
}

// XCD-aware tile order for the pair kernels (1-D grids).  The dispatcher hands workgroups to the 8 XCDs round-robin by
// flat id, and every XCD has its own 4 MiB L2.  With a plain 2-D grid each XCD sees tiles from everywhere and streams
// the whole bitmap (plus rank and entry tables) through its L2 again and again: at N = 20,000 the popcount kernel
// fetched 2.4 GB for a 12.6 MB bitmap, the walker 11 GB (profiles/r02/experiments/c_counters.json).  Here tiles are grouped into
// super-tiles of up to 8 x 8 tiles and consecutive workgroups of one XCD walk one super-tile, so the ~100 workgroups
// resident on an XCD share the rows of one or two super-tiles (0.29 GB and 1.3 GB after the change).  Affinity only:
// nothing depends on where a workgroup really runs.
// Super-tile edge: 8 tiles (16 for k_sparse_tile64, whose tiles re-read 800 B of entry lists per row: 0.84 -> 0.56 GB fetched at
// N = 20,000; for the popcount tiles and the walker 16 changed nothing measurable), halved while that would leave an XCD with
// fewer than 16 super-tiles (small matrices must
// still spread over all 8 XCDs; at edge 1 the deal is tile by tile).
__host__ __device__ __forceinline__ unsigned pc_super_edge(unsigned ntx, unsigned nty, unsigned top = 8) {
    unsigned e = top;
    while (e > 1 && ((ntx + e - 1) / e) * ((nty + e - 1) / e) < 128u) e >>= 1;
    return e;
}
// XCD x takes, in super-tile row sy, the columns sx = 8c + ((x - sy) mod 8): every XCD gets every eighth super-tile of
// each row AND of each column, so the triangular (or, for a shard, trapezoid) region of live tiles is dealt evenly --
// dealing whole columns to XCDs left them 40 % apart on the triangle.
__device__ __forceinline__ bool pc_tile_of_index(unsigned n, int ntx, int nty, int& tx, int& ty, unsigned top = 8) {
    const unsigned e = pc_super_edge((unsigned)ntx, (unsigned)nty, top);
    const unsigned xcd = n & 7u, k = n >> 3;
    const unsigned stx = ((unsigned)ntx + e - 1) / e, stx8 = (stx + 7u) / 8u;
    const unsigned m = k / (e * e), within = k % (e * e);
    const unsigned sy = m / stx8, c = m % stx8;
    const unsigned sx = c * 8u + ((xcd + 8u - (sy & 7u)) & 7u);
    tx = (int)(sx * e + within % e);
    ty = (int)(sy * e + within / e);
    return tx < ntx && ty < nty;
}
__device__ __forceinline__ bool pc_tile_of_block(int ntx, int nty, int& tx, int& ty, unsigned top = 8) { return pc_tile_of_index(blockIdx.x, ntx, nty, tx, ty, top); }
static unsigned pc_tile_grid(int ntx, int nty, unsigned top = 8) {
    const unsigned e = pc_super_edge((unsigned)ntx, (unsigned)nty, top);
    const unsigned stx = ((unsigned)ntx + e - 1) / e, sty = ((unsigned)nty + e - 1) / e;
    return sty * ((stx + 7u) / 8u) * 8u * e * e;
}

// shared: |S n T| (gcs, jc) or the conserved gene count sum over shared phams of cnt_s + cnt_t (pocp); tot: nph_s + nph_t, resp. ngen_s + ngen_t
template <int METRIC>
__device__ __forceinline__ double pc_set_value(int shared, int tot, int as_distance) {
    double sim = 0.0;
    if (shared) {
        if (METRIC == PC_GCS) sim = (2.0 * (double)shared) / (double)tot;      // metrics.py:45-48
        else if (METRIC == PC_JC) sim = (double)shared / (double)(tot - shared);   // metrics.py:75
        else sim = (double)shared / (double)tot;                                 // metrics.py:104-110
    }
    return pc_finish(sim, as_distance);
}

// target genome of shard slot k (an unsharded context owns every genome in order: no table read on the critical path)
__device__ __forceinline__ int pc_owned(const PcShard& sh, int k) { return sh.ident ? k : sh.owned[k]; }

// The launchers' template dispatch: f(m as a std::integral_constant) for m among M0, MS...; false: m is none of them.  Each launcher
// names the instances of its kernel once.
template <int M0, int... MS, class F>
static bool pc_dispatch(int m, F&& f) {
    if (m == M0) { f(std::integral_constant<int, M0>{}); return true; }
    if constexpr (sizeof...(MS) > 0) return pc_dispatch<MS...>(m, f);
    return false;
}

static int pc_metric_of_mode(int mode) { return mode == PCW_SPARSE_GCS ? PC_GCS : mode == PCW_SPARSE_JC ? PC_JC : mode == PCW_POCP ? PC_POCP : PC_AF; }

// ---------------------------------------------------------------------------------
// Constants that both a kernel and pc_set_shape_of read, family by family (what they mean is told where the kernels are).
// ---------------------------------------------------------------------------------
// k_set_popc: live 64x64 tiles below which the popcount kernel switches to the word-split 32x32 kernel (measured, jc device time, 64-tile vs
// word-split: N = 1,000 26.7 / 18.8 us, 2,000 53.6 / 35.8, 3,000 74.6 / 69.0, 5,000 157 / 167: profiles/r03/experiments/a_popc_tile_ab.txt)
#define PC_SMALL_GRID_TILES 1536
#define SP_T 32                                                   // k_sparse_tile: tile edge (genomes); masks are one u32
#define S6_T 64                                                   // k_sparse_tile64 and k_sparse_col: tile edge; masks are two u32
#define S6_LD 65                                                  // row stride of their u32 accumulators in LDS
#define S6_WAVES 8
#define S6_GCS PCW_SPARSE_GCS                                     // MODE values beside PCW_POCP / PCW_AF: shared-pham counts only (gcs, jc)
#define S6_JC PCW_SPARSE_JC
#define S6_SUPER 16                                               // super-tile edge in tiles: 2 x 1,024 rows' entry lists = 1.6 MB of an XCD's 4-MB L2
// af: a probe step with at least this many broadcast entries takes them through LDS instead of the readlane loop (k_sparse_tile64).  Measured
// (profiles/r04/experiments/dense_broadcast_af.txt; af at N = 2,000): threshold 4: 0.120 ms, 8: 0.098, 12: 0.0905, 24: 0.0894; never: 0.127
#ifndef S6_DENSE_MIN
#define S6_DENSE_MIN 24
#endif
#define S6_STAGE_DWORDS 192                                       // per wave: 64 x (mask low, mask high, value)
// Which instances take it: af's two-batch one (small and medium collections, 128 registers).  The one-batch instances sit at 78-79 of
// the 80 registers six waves per SIMD leave and spilled 8-12 dwords with it (scratch stores reach HBM); pocp's two-batch instance
// spilled 24; the counting mode keeps its four workgroups per CU -- no LDS to spare.
__host__ __device__ constexpr bool pc_s6_dense(int mode, int batches) { return S6_DENSE_MIN > 0 && mode == PCW_AF && batches == 2; }
#define S7_SEG 8                                                  // k_sparse_col: source tiles per unit, at most (small matrices: fewer, see the launcher)
