// pc_nw_geometry.h -- what the K4 kernels (pc_nw_systolic.h), the host's launch arithmetic (pc_nw_shape.hip) and the planner (pc_plan.hip,
// pc_upload.hip) agree on, each stated once: the constants that size a workgroup and the geometry of a column gene on a variant.
// Constants and __host__ __device__ constexpr helpers only: no kernel, no __constant__ table, no inline asm.
#pragma once
#include "pc_common.h"

#define PC_MAX_SEG 16                               // most segments (row streams) a wave carries
#define PC_WIN 32                                   // stream entries staged per refill (one segment per 64-lane pass; 64 was measured: no gain)
#define PC_WG_HEADER_DWORDS 144                     // head of a workgroup's LDS: the 24 x 24 score table, a byte per entry

// ---- the geometry: a column gene of lb residues on a variant of W columns per lane
__host__ __device__ constexpr int pc_nw_lanes(int lb, int W) { return (lb + W - 1) / W; }                 // lanes per segment, G
// segments per wave of a segment of G lanes, and of (lb, W); strip-mined genes (G > 64): one row per wave
__host__ __device__ constexpr int pc_nw_segs_of(int G) { return G > 64 ? 1 : (64 / G > PC_MAX_SEG ? PC_MAX_SEG : 64 / G); }
__host__ __device__ constexpr int pc_nw_segs(int lb, int W) { return pc_nw_segs_of(pc_nw_lanes(lb, W)); }
// Lanes-per-segment bucket of a launch class (bound 8, 16, 32, 64; index 0..3): every column gene of a launch lies in one
// bucket, so launch, task sizes and LDS agree on the waves per workgroup without passing it around
__host__ __device__ constexpr int pc_nw_g_index(int G) { return G <= 8 ? 0 : (G <= 16 ? 1 : (G <= 32 ? 2 : 3)); }
__host__ __device__ constexpr int pc_nw_g_bucket(int G) { return 8 << pc_nw_g_index(G); }
// lanes per segment of a launch's longest column gene, within what a wave has (a strip-mined launch: all 64)
__host__ __device__ constexpr int pc_nw_launch_lanes(int max_lb, int W) { return pc_nw_lanes(max_lb, W) > 64 ? 64 : (pc_nw_lanes(max_lb, W) < 1 ? 1 : pc_nw_lanes(max_lb, W)); }
// PC_MODE_* of a task of `rows` rows on a variant with nseg segments per wave: all rows in one wave's segments, in two waves', or
// the class's own workgroup (T: the integer type the caller counts rows in -- the device planner's is unsigned)
template <class T> __host__ __device__ constexpr int pc_nw_mode_of(T rows, T nseg) { return rows <= nseg ? PC_MODE_ONE_WAVE : (rows <= 2 * nseg ? PC_MODE_TWO_WAVES : PC_MODE_CLASS); }

// Every variant up to this W exists twice.  INC16: the statistics' increment comes from a second, 16-bit profile, 10
// instructions per cell, 3 x the LDS; the other compares residues, 11 instructions.  The launcher picks per launch
// class (pc_nw_class_inc16): the big profile pays while four waves per SIMD still fit beside it.
#define PC_INC16_MAX_W 24
__host__ __device__ constexpr int pc_prof_rows(bool inc16) { return inc16 ? 25 : 24; }
__host__ __device__ constexpr int pc_prof_row_dwords(int W, bool inc16) {   // scores (4 per dword), then increments (2 per dword)
    return (W + 3) / 4 + (inc16 ? (W + 1) / 2 : 0);
}

// Waves per workgroup, sharing one profile: 4, or 8 where the profile of a longer column gene would otherwise leave
// fewer than four waves per SIMD in the CU's 160 KB of LDS (chosen per launch class by pc_nw_class_waves; the kernel
// reads it from blockDim).  16-wave workgroups were tried for segments of 64 lanes: one workgroup per CU, 5-10 % slower
// than the residue-compare cell with its small profile, which those classes run instead.
#define PC_MIN_WAVES 4
__host__ __device__ constexpr int pc_max_waves(int W) { return W <= 24 ? 8 : 4; }
__host__ __device__ constexpr int pc_wave_lds_dwords(int nseg) { return 4 * 64 + 2 * PC_MAX_SEG + nseg * PC_WIN; }   // private LDS of a wave with nseg row streams

// ---- the strip-mined kernel (k_nw_strip)
#define PC_STRIP_WAVES 4                                           // most waves per workgroup = rows per task (one row per wave)
#define PC_STRIP_WIN 32                                            // stream entries a strip wave stages per refill (the idle half of the wave stages the boundary line: fixed)
#define PC_STRIP_BND 64                                            // boundary entries a wave keeps staged (two refill windows)
__host__ __device__ constexpr int pc_strip_wave_lds_dwords() { return 16 + PC_STRIP_WIN + 4 * PC_STRIP_BND; }
#define PC_PIPE_WAVES_MAX 8                                        // most waves of its PIPE form (the passes of one alignment over the waves)
// scratch of one resident workgroup: a boundary line of (longest row + 2) 16-byte entries per wave
__host__ __device__ constexpr size_t pc_strip_block_bytes(int max_row_len, int nw) { return (size_t)nw * ((size_t)max_row_len + 2) * 16; }
// the strip-mined kernel's widths: the wide variants for tasks of 3-4 rows (four waves share the profile of a pass), W = 12 / W = 8
// for tasks of two rows / one row -- the profile of a pass is 24 x W x 64 bytes of LDS PER COLUMN GENE, 49 KB at W = 32: with one
// row to align against it a CU would hold three waves; at W = 8 it holds twelve, for 9 % more instructions per cell
#define PC_STRIP_W_ONE_ROW 8
#define PC_STRIP_W_TWO_ROWS 12

// tiers by registers (waves per SIMD): 2..8 (<= 72: seven or more), 9..12 (<= 92: five), 13..19 (<= 128: four), 20..24 (<= 152: three)
#define PC_NUM_TIERS 4
__host__ __device__ constexpr int pc_tier_of(int W) { return W <= 8 ? 0 : W <= 12 ? 1 : W <= 19 ? 2 : W <= 24 ? 3 : -1; }
