// pc_sparse.hip -- pocp / af (and, on the 64x64 tiles, gcs / jc) as a SPARSE bitset intersection: the work follows a pair's shared
// phams instead of the words of its bitmap rows.  k_sparse_tile (32x32 tiles, small matrices), k_sparse_tile64 (64x64 tiles, row-per-wave
// probes), and the upload-time kernels that make their entry lists (k_pair_entries, k_sp_build).
//
// Reference semantics restated here (metrics.py of the reference):
//   metrics.py:102-110    pocp = conserved gene count / (ngen_s + ngen_t)
//   metrics.py:135-152    af = conserved length / (tlen_s + tlen_t)
//   metrics.py:45-53, 75-80   gcs / jc through pc_set_value (pc_pairs.h)
#include "pc_pairs.h"

// K2 for SMALL matrices: pocp / af as a SPARSE bitset intersection (r03).  Used below ~3,500 genomes, where it beats the
// shared-pham walker (N = 2,000: 0.122 against 0.184 ms); above, the walker stays (N = 20,000: 5.6 against 7.1 ms --
// where the time goes: `profiles/r03/experiments/c_sparse_tile_experiment.txt`: the divergent per-bit add loops 3.6 ms, mask build + reads
// 2.9 ms, everything else, fp64 epilogue included, 0.7 ms).
//
// A genome holds ~100 of the P = 5,000 phams, a pair shares ~3 of them, and pocp / af need a value per SHARED pham
// (gene count, summed length: metrics.py:102-103, 135-147).  The walker scans all W words of both bitmap rows per pair
// and then chases rank table -> entry table for every hit: 2.8 x the popcount kernel, 3.5 % of HBM speed at N = 20,000.
// Here the work follows the shared phams instead of the words.  One workgroup owns a 32 x 32 tile of pairs and
//   A. transposes the tile's 32 TARGET bitmap rows into LDS: colmask[p] = which of the 32 targets hold pham p (built
//      from the targets' entry lists -- the set bits of their rows -- with LDS atomic ORs),
//   B. lets every entry (p, v) of the 32 SOURCE rows look up colmask[p] and add v into acc[source][target] for each set
//      bit (LDS atomic adds; 64-bit: value in the low 40 bits, a hit count above them, so "no shared pham" stays
//      distinguishable from "shared phams of total value 0"),
//   C. does the same with the roles swapped (colmask over the sources, the targets' entries probe), and
//   D. finishes each pair: (sum_s + sum_t) / (total_s + total_t), 1 - x, round(., 6) in fp64, one coalesced store.
// Per pair that is ~2 x 6 entry visits + ~6 atomic adds + the epilogue instead of 79 word scans + the visits.  Phams are
// processed in chunks of CH (the colmask array is CH words of dynamic LDS), entry ranges of a chunk come from the rank
// table (rankpre is the entry index at every 64-pham word boundary).  No MFMA: there is no dense contraction, and at 2 %
// density a dense one would do 50 x the work.
#define SP_IT 16                                                  // entries a lane loads per batch (8 lanes per row: 128 entries of a row)
template <int MODE>
__global__ __launch_bounds__(256) void k_sparse_tile(PcDev d, PcShard sh, double* __restrict__ out, int as_distance, int condensed, int CH) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];
    uint32_t* colmask = sp_lds;                                                    // [CH]
    unsigned long long* acc = (unsigned long long*)(sp_lds + CH);                  // [32 sources][32 targets]  (CH is even: 8-byte aligned)
    __shared__ int g_s[SP_T], g_t[SP_T];                                           // genome of tile row r, -1: none
    int tile_x, tile_y;
    if (!pc_tile_of_block((d.N + SP_T - 1) / SP_T, (sh.nown + SP_T - 1) / SP_T, tile_x, tile_y)) return;
    const int s0 = tile_x * SP_T, k0 = tile_y * SP_T;
    const int klast = min(k0 + SP_T, sh.nown) - 1;
    if (s0 >= pc_owned(sh, klast)) return;
    if (threadIdx.x < SP_T) {
        const int s = s0 + threadIdx.x, k = k0 + threadIdx.x;
        g_s[threadIdx.x] = s < d.N ? s : -1;
        g_t[threadIdx.x] = k < sh.nown ? pc_owned(sh, k) : -1;
    }
    for (int i = threadIdx.x; i < SP_T * SP_T; i += 256) acc[i] = 0ULL;
    // a row's entries go to 8 consecutive lanes: lane (row = tid >> 3, sub = tid & 7) takes entries sub, sub + 8, ...
    // Every phase first issues ALL its global loads (SP_IT independent loads per lane and array: one memory latency per
    // phase, not one per entry -- with the loads inside the loops a tile took 52 of them back to back and the kernel was
    // slower than the walker), then works on LDS only.
    const int row = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const uint2* __restrict__ ent = MODE == PCW_POCP ? d.ent_pair_cnt : d.ent_pair_len;
    for (int p0 = 0; p0 < d.Wb * 64; p0 += CH) {
        const int w0 = p0 >> 6, w1 = min(d.Wb, (p0 + CH) >> 6);
        __syncthreads();                                                            // g_s, g_t, acc visible / previous chunk done
        uint32_t ebs = 0, ees = 0, ebt = 0, eet = 0;                                // my rows' entries of this chunk
        if (g_s[row] >= 0) {
            ebs = d.rankpre[(int64_t)g_s[row] * d.Wb + w0];
            ees = w1 < d.Wb ? d.rankpre[(int64_t)g_s[row] * d.Wb + w1] : d.ent_off[g_s[row] + 1];
        }
        if (g_t[row] >= 0) {
            ebt = d.rankpre[(int64_t)g_t[row] * d.Wb + w0];
            eet = w1 < d.Wb ? d.rankpre[(int64_t)g_t[row] * d.Wb + w1] : d.ent_off[g_t[row] + 1];
        }
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            // pass 0: masks over the targets, the sources' entries probe; pass 1: the other way round
            const uint32_t bb = pass == 0 ? ebt : ebs, be = pass == 0 ? eet : ees;  // rows that BUILD the masks
            const uint32_t qb = pass == 0 ? ebs : ebt, qe = pass == 0 ? ees : eet;  // rows that PROBE them
            if (pass) __syncthreads();                                              // previous probes done
            for (int i = threadIdx.x * 4; i < CH; i += 1024) *(uint4*)&colmask[i] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            for (uint32_t e0 = bb + sub; e0 < be; e0 += 8 * SP_IT) {
                int ph[SP_IT];
#pragma unroll
                for (int i = 0; i < SP_IT; ++i) ph[i] = e0 + 8 * i < be ? d.ent_pham[e0 + 8 * i] - p0 : -1;
#pragma unroll
                for (int i = 0; i < SP_IT; ++i) if (ph[i] >= 0) atomicOr(&colmask[ph[i]], 1u << row);
            }
            __syncthreads();
            for (uint32_t e0 = qb + sub; e0 < qe; e0 += 8 * SP_IT) {
                int ph[SP_IT]; uint32_t vv[SP_IT], mm[SP_IT];
#pragma unroll
                for (int i = 0; i < SP_IT; ++i) {                                   // (pham, value) in one 8-byte load
                    const uint2 x = e0 + 8 * i < qe ? ent[e0 + 8 * i] : make_uint2((uint32_t)(p0 - 1), 0u);
                    ph[i] = (int)x.x - p0;
                    vv[i] = x.y;
                }
#pragma unroll
                for (int i = 0; i < SP_IT; ++i) mm[i] = ph[i] >= 0 ? colmask[ph[i]] : 0u;
#pragma unroll
                for (int i = 0; i < SP_IT; ++i) {
                    uint32_t m = mm[i];
                    const unsigned long long v = (1ULL << 40) | (unsigned long long)vv[i];
                    while (m) {
                        const int o = __ffs((int)m) - 1;
                        m &= m - 1;
                        atomicAdd(&acc[pass == 0 ? row * SP_T + o : o * SP_T + row], v);
                    }
                }
            }
        }
    }
    __syncthreads();
    // finish: 1,024 pairs, 4 per thread; consecutive lanes run along the output's contiguous direction
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = threadIdx.x + 256 * q;
        const int fast = idx & 31, slow = idx >> 5;
        const int ls = condensed ? slow : fast, lt = condensed ? fast : slow;
        const int s = g_s[ls], t = g_t[lt];
        if (s < 0 || t < 0 || s >= t) continue;
        const unsigned long long a = acc[ls * SP_T + lt];
        const bool any = (a >> 40) != 0;
        const long long cons = (long long)(a & ((1ULL << 40) - 1));
        double sim = 0.0;
        if (any) {
            if (MODE == PCW_POCP) sim = (double)cons / (double)(d.ngen[s] + d.ngen[t]);    // metrics.py:104-110
            else sim = (double)cons / (double)(d.tlen[s] + d.tlen[t]);                      // metrics.py:149-152
        }
        out[pc_out_index(d, sh, s, t, k0 + lt, condensed)] = pc_finish(sim, as_distance);
    }
}

int pc_launch_sparse(int mode, const PcDev& d, const PcShard& sh, double* out, int as_distance, int condensed, hipStream_t st, pc_set_shape* shape_out) {
    pc_set_shape shp;
    pc_set_shape_of(K_SPARSE32, pc_metric_of_mode(mode), d.N, sh.nown, d.Wb, d.sp_W, d.n_cu, 0, pc_set_knobs_env(), &shp);
    if (shape_out) *shape_out = shp;
    if (sh.nown <= 0 || d.N <= 1) return PC_OK;
    const int CH = shp.chunk;
    const size_t lds = (size_t)shp.lds;
    dim3 grid((unsigned)shp.grid), block(256);
    if (!pc_dispatch<PCW_POCP, PCW_AF>(mode, [&](auto m) { hipLaunchKernelGGL(k_sparse_tile<decltype(m)::value>, grid, block, lds, st, d, sh, out, as_distance, condensed, CH); })) {
        pc_set_error("pc_launch_sparse: bad mode %d", mode); return PC_ERR_ARG;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_sparse_tile launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// ---------------------------------------------------------------------------------
// K2 for LARGE matrices (r03): the sparse formulation again, on 64 x 64 tiles with row-per-wave probes.
//
// What kept the 32 x 32 kernel behind the walker at N = 20,000 (profiles/r03/experiments/c_sparse_tile_experiment.txt): a tile pays for
// 4 x 32 entry lists (build + probe, both directions) whatever its 1,024 pairs share, and its per-bit add loops diverge --
// most probes of a source row hit no target or one, a few (phams of the target cluster's pool) hit twenty, and a wave
// runs the longest loop of its 64 lanes.  Here
//   * a tile is 64 x 64 pairs (masks are two u32 per pham): the list work per pair halves;
//   * eight waves; a wave owns eight rows of either side and loads ALL their entries (128 per row) into registers with
//     one round of coalesced loads at the start of the tile -- one memory latency per tile, not one per phase (a first
//     version that fetched row after row spent 3.0 of its 7.5 ms waiting for them);
//   * masks are built and probed from those registers; a wave probes ONE row at a time, 64 of its entries per step;
//   * a probe that hits at most two rows of the other side adds them itself (LDS atomics, two short iterations);
//   * a probe that hits more is BROADCAST (readlane): its 64-bit mask becomes the EXEC mask of one v_add into a register
//     the 64 lanes hold for the 64 rows of the other side -- no divergence, no LDS traffic; the register is flushed into
//     the LDS accumulators once per probing row.
//   * an entry is ONE 8-byte load: (pham, value) pairs, made on the device at upload (k_pair_entries); the epilogue's
//     denominators come from LDS (64 + 64 totals per tile);
//   * pocp adds count + 1 where the sources probe and count - 1 where the targets do, so in the second direction only the
//     targets' paralog entries (~6 %) probe at all.
// Accumulators: u32 in LDS, row stride 65 (both directions conflict free).  "No shared pham" is "sum == 0": the host uses
// this kernel only when every entry value is >= 1 (always true for gene counts; for summed lengths unless a translation
// is empty) and every genome's total stays below 2^31 -- otherwise the 32 x 32 kernel / the walker (af) or the popcount
// tiles (pocp) run.
// ---------------------------------------------------------------------------------
#define S6_RPW (S6_T / S6_WAVES)                                  // rows (of either side) a wave owns
// S6_B: 64-entry batches of a row held in registers -- 2 when one mask chunk holds all phams (a row's ~100 entries), 1 when the
// phams take several chunks (a row then has a few dozen entries per chunk; half the loads and probe steps, and registers for a
// third workgroup per CU: the launch bound asks for six waves per SIMD there)
// Waves per SIMD the instances are compiled for.  The counting mode's one-batch instance takes 59 registers: eight waves per SIMD,
// FOUR workgroups per CU beside 4 x 38.6 KB of LDS (r04: N = 20,000 jc 1.78 -> 1.56 ms -- a tile is a chain of latencies, three
// global-load rounds and five barriers, so what a CU overlaps is what counts).  af / pocp need 78-79 and stay at six (three
// workgroups); what was tried to get them to 64 and was slower or spilled (profiles/r04/experiments/sparse64_occupancy.txt):
// 16-wave tiles with four rows per wave (64 registers with 9-12 dwords of scratch: pocp 2.38 -> 2.87 ms, af 2.58 -> 2.99), one
// register per entry (13 bits of id, 19 of value: the compiler unpacks up front or spills 17-31 dwords under the 64 bound).
__host__ __device__ constexpr int pc_s6_waves_per_simd(int mode, int batches) { return batches != 1 ? 4 : (mode >= PCW_SPARSE_GCS ? 8 : 6); }
template <int MODE, int S6_B>
__global__ __launch_bounds__(64 * S6_WAVES, pc_s6_waves_per_simd(MODE, S6_B)) void k_sparse_tile64(PcDev d, PcShard sh, double* __restrict__ out, int as_distance, int condensed, int CH, unsigned n_units) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];
    uint32_t* colmask = sp_lds;                                                    // [CH][2]
    uint32_t* acc = sp_lds + 2 * CH;                                               // [64 sources][65]
    __shared__ int g_s[S6_T], g_t[S6_T];                                           // genome of tile row r, -1: none
    __shared__ long long tot_s[S6_T], tot_t[S6_T];                                 // its total (genes, resp. residues): the epilogue's denominators
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t* stage = acc + S6_T * S6_LD + wave * S6_STAGE_DWORDS;                 // af / pocp: this wave's broadcast entries (pc_s6_dense)
    constexpr bool COUNT = MODE >= S6_GCS;                                          // gcs / jc: |S n T| only -- every hit adds 1, and ONE direction does it
    const uint2* __restrict__ ent = MODE == PCW_POCP ? d.sp_cnt : d.sp_len;                   // (dense pham id, value): phams with at least two holders
    // Unit n of the XCD-aware tile order goes to workgroup n mod gridDim (a multiple of 8, so a workgroup keeps to the tiles of
    // its XCD).  Tiles differ in cost by 10 x (a tile inside a cluster of related genomes shares ~85 phams per pair, one between
    // clusters ~3), so the deal must stay fine: measured at N = 20,000 with gridDim = m x the 512 resident workgroups, m = 1: 4.40 ms,
    // 8: 3.73, 64: 3.37 (a workgroup then takes ~3 units, half of them below the diagonal), one workgroup per unit: 3.51;
    // N = 8,000: best at m = 16, again ~3 units each.  Hence gridDim = units / 3.
#pragma unroll 1
    for (unsigned unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
    int tile_x, tile_y;
    if (!pc_tile_of_index(unit, (d.N + S6_T - 1) / S6_T, (sh.nown + S6_T - 1) / S6_T, tile_x, tile_y, S6_SUPER)) continue;
    const int s0 = tile_x * S6_T, k0 = tile_y * S6_T;
    const int klast = min(k0 + S6_T, sh.nown) - 1;
    if (s0 >= pc_owned(sh, klast)) continue;
    // lane l looks at row l of either side: genome, then (per chunk) where its entries start and end
    const int gs_l = s0 + lane < d.N ? s0 + lane : -1, gt_l = k0 + lane < sh.nown ? pc_owned(sh, k0 + lane) : -1;
    if (wave == 0) {
        g_s[lane] = gs_l; g_t[lane] = gt_l;
        tot_s[lane] = gs_l < 0 ? 0 : (COUNT ? (long long)d.nph[gs_l] : MODE == PCW_POCP ? (long long)d.ngen[gs_l] : (long long)d.tlen[gs_l]);
        tot_t[lane] = gt_l < 0 ? 0 : (COUNT ? (long long)d.nph[gt_l] : MODE == PCW_POCP ? (long long)d.ngen[gt_l] : (long long)d.tlen[gt_l]);
    }
    for (int i = tid; i < S6_T * S6_LD; i += 64 * S6_WAVES) acc[i] = 0u;
    for (int p0 = 0; p0 < d.sp_W * 64; p0 += CH) {
        const int w0 = p0 >> 6, w1 = min(d.sp_W, (p0 + CH) >> 6);
        // my rows' entries of this chunk, sources and targets: ranges (wave-uniform), then 2 x 64 entries per row in registers
        uint32_t rl_s = 0, rh_s = 0, rl_t = 0, rh_t = 0;
        if (gs_l >= 0) { rl_s = d.sp_rank[(int64_t)gs_l * d.sp_W + w0]; rh_s = w1 < d.sp_W ? d.sp_rank[(int64_t)gs_l * d.sp_W + w1] : d.sp_end[gs_l]; }
        if (gt_l >= 0) { rl_t = d.sp_rank[(int64_t)gt_l * d.sp_W + w0]; rh_t = w1 < d.sp_W ? d.sp_rank[(int64_t)gt_l * d.sp_W + w1] : d.sp_end[gt_l]; }
        uint32_t lo_s[S6_RPW], hi_s[S6_RPW], lo_t[S6_RPW], hi_t[S6_RPW];
#pragma unroll
        for (int rr = 0; rr < S6_RPW; ++rr) {
            const int r = wave + S6_WAVES * rr;
            lo_s[rr] = (uint32_t)__builtin_amdgcn_readlane((int)rl_s, r); hi_s[rr] = (uint32_t)__builtin_amdgcn_readlane((int)rh_s, r);
            lo_t[rr] = (uint32_t)__builtin_amdgcn_readlane((int)rl_t, r); hi_t[rr] = (uint32_t)__builtin_amdgcn_readlane((int)rh_t, r);
        }
        // pocp keeps BOTH sides' gene counts of slot (rr, b) in one register (source's count below, target's above bit 16: the host
        // takes this kernel for pocp only while every genome holds fewer than 65,536 genes).  With a register each, the one-batch
        // instance needed 84 against the 80 that six waves per SIMD leave: three dwords went to scratch, and scratch stores reach
        // HBM -- the 23 % of writes beyond the matrix that the r03 counters showed for pocp alone (WRITE_SIZE 1.97 GB for 1.60 GB)
        constexpr bool PACKED = MODE == PCW_POCP;
        int ph_s[S6_RPW][S6_B], ph_t[S6_RPW][S6_B]; uint32_t v_s[S6_RPW][S6_B], v_t[PACKED ? 1 : S6_RPW][PACKED ? 1 : S6_B];
#pragma unroll
        for (int rr = 0; rr < S6_RPW; ++rr)
#pragma unroll
            for (int b = 0; b < S6_B; ++b) {
                const uint32_t es = lo_s[rr] + (uint32_t)(64 * b + lane), et = lo_t[rr] + (uint32_t)(64 * b + lane);
                const bool is = es < hi_s[rr], it = et < hi_t[rr];
                if constexpr (COUNT) {
                    ph_s[rr][b] = is ? d.sp_pham[es] - p0 : -1; v_s[rr][b] = 1u;
                    ph_t[rr][b] = it ? d.sp_pham[et] - p0 : -1; v_t[rr][b] = 1u;
                } else {
                    const uint2 xs = is ? ent[es] : make_uint2((uint32_t)(p0 - 1), 0u), xt = it ? ent[et] : make_uint2((uint32_t)(p0 - 1), 0u);
                    ph_s[rr][b] = (int)xs.x - p0; ph_t[rr][b] = (int)xt.x - p0;
                    if constexpr (PACKED) v_s[rr][b] = xs.y | (xt.y << 16);
                    else { v_s[rr][b] = xs.y; v_t[rr][b] = xt.y; }
                }
            }
        // one direction: the rows of one side build the masks, the rows of the other probe them.  TO_ROW: the probing rows are
        // the accumulator rows (sources probe), else its columns (targets probe)
        auto hit = [&](auto to_row, auto packed, int r, int ph, uint32_t v, uint32_t& hs) {
            // pocp: the entry's gene count c adds c + 1 where the sources probe and c - 1 where the targets do (see below)
            if constexpr (MODE == PCW_POCP) {
                if constexpr (decltype(packed)::value) v = decltype(to_row)::value ? (v & 0xffffu) : (v >> 16);
                v = decltype(to_row)::value ? v + 1u : v - 1u;
            }
            uint2 m = make_uint2(0u, 0u);
            if (ph >= 0) m = *(const uint2*)&colmask[2 * ph];
            const int pc = __popc(m.x) + __popc(m.y);
            if (pc > 0 && pc <= 2) {                                                // one or two hits: this lane adds them
                const unsigned long long mm = ((unsigned long long)m.y << 32) | m.x;
                const int o1 = __builtin_ctzll(mm), o2 = 63 - __builtin_clzll(mm);
                atomicAdd(&acc[decltype(to_row)::value ? r * S6_LD + o1 : o1 * S6_LD + r], v);
                if (pc == 2) atomicAdd(&acc[decltype(to_row)::value ? r * S6_LD + o2 : o2 * S6_LD + r], v);
            }
            unsigned long long heavy = __ballot(pc > 2);                            // many hits: the wave adds them, lanes = rows of the other side
            if constexpr (pc_s6_dense(MODE, S6_B)) {
                // Inside a cluster nearly every entry is such a hit (a pair shares ~85 phams), and the loop below takes ~10 instructions
                // and a VALU -> SGPR -> EXEC round trip per entry: the launch lasted as long as its slowest in-cluster tile.  Dense
                // form (r04): the 64 entries go to LDS (mask halves and value; zero where the lane's entry is not a broadcast one), and
                // lane l walks all 64 -- its own half of the mask by a broadcast read -- adding the value where its bit is set: two LDS
                // reads and two VALU instructions per entry, no scalar dependency, iterations independent.
                if (__popcll(heavy) >= S6_DENSE_MIN) {
                    const bool big = pc > 2;
                    stage[lane] = big ? m.x : 0u; stage[64 + lane] = big ? m.y : 0u; stage[128 + lane] = v;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the wave's own LDS writes -> its reads (in-order LDS queue)
                    uint32_t l2 = (uint32_t)lane;
                    asm volatile("" : "+v"(l2));                                    // (derived per step: hoisted out of the unrolled rows, `mine` and `sh` cost the one-batch instances 8-12 dwords of scratch)
                    const uint32_t* mine = stage + (l2 & 32u) * 2u;                 // lanes 0-31: low halves, 32-63: high halves
                    const uint32_t sh = l2 & 31u;
#pragma unroll 8
                    for (int k = 0; k < 64; ++k) hs += ((mine[k] >> sh) & 1u) * stage[128 + k];
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // reads done before the next step rewrites the stage
                    heavy = 0;
                }
            }
            while (heavy) {
                const int k = __builtin_ctzll(heavy);
                asm("s_bitset0_b64 %0, %1" : "+s"(heavy) : "s"(k));
                const unsigned long long mk = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)m.y, k) << 32) |
                                              (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)m.x, k);
                const uint32_t vk = (uint32_t)__builtin_amdgcn_readlane((int)v, k);
                // (every lane of the workgroup is active here -- 512 threads, wave-uniform control flow -- so EXEC is all ones before and after)
                asm volatile("s_mov_b64 exec, %1\n\tv_add_u32 %0, %0, %2\n\ts_mov_b64 exec, -1" : "+v"(hs) : "s"(mk), "s"(vk));
            }
        };
        auto direction = [&](auto to_row, const int (&bph)[S6_RPW][S6_B], const uint32_t (&blo)[S6_RPW], const uint32_t (&bhi)[S6_RPW],
                             const int (&qph)[S6_RPW][S6_B], const uint32_t (&qv)[S6_RPW][S6_B], const uint32_t (&qlo)[S6_RPW], const uint32_t (&qhi)[S6_RPW]) {
            for (int i = tid * 4; i < 2 * CH; i += 256 * S6_WAVES) *(uint4*)&colmask[i] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < S6_RPW; ++rr) {
                const int r = wave + S6_WAVES * rr;
                const uint32_t bit = 1u << (r & 31); const int half = r >> 5;
#pragma unroll
                for (int b = 0; b < S6_B; ++b) if (bph[rr][b] >= 0) atomicOr(&colmask[2 * bph[rr][b] + half], bit);
                for (uint32_t e0 = blo[rr] + 64u * S6_B; e0 < bhi[rr]; e0 += 64u) {          // rows with more entries than the registers hold
                    const uint32_t e = e0 + (uint32_t)lane;
                    if (e < bhi[rr]) atomicOr(&colmask[2 * (d.sp_pham[e] - p0) + half], bit);
                }
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < S6_RPW; ++rr) {
                const int r = wave + S6_WAVES * rr;
                uint32_t hs = 0;
#pragma unroll
                for (int b = 0; b < S6_B; ++b) hit(to_row, std::integral_constant<bool, PACKED>{}, r, qph[rr][b], qv[rr][b], hs);
                for (uint32_t e0 = qlo[rr] + 64u * S6_B; e0 < qhi[rr]; e0 += 64u) {
                    const uint32_t e = e0 + (uint32_t)lane;
                    const bool in = e < qhi[rr];
                    uint2 x = make_uint2((uint32_t)(p0 - 1), 0u);
                    if (in) { if constexpr (COUNT) x = make_uint2((uint32_t)d.sp_pham[e], 1u); else x = ent[e]; }
                    hit(to_row, std::false_type{}, r, (MODE == PCW_POCP && !decltype(to_row)::value && x.y <= 1u) ? -1 : (int)x.x - p0, x.y, hs);
                }
                if (hs) atomicAdd(&acc[decltype(to_row)::value ? r * S6_LD + lane : lane * S6_LD + r], hs);
            }
            __syncthreads();                                                        // probes done before the masks are cleared again
        };
        direction(std::true_type{}, ph_t, lo_t, hi_t, ph_s, v_s, lo_s, hi_s);       // masks over the targets, the sources' entries probe
        if constexpr (COUNT) {
            // |S n T| is symmetric: the sources' probes have counted it
        } else if constexpr (MODE == PCW_POCP) {
            // conserved(s, t) = sum over shared phams of cnt_s + cnt_t = sum (cnt_s + 1) + sum (cnt_t - 1): the first direction added
            // cnt_s + 1 per hit; in the second only the targets' PARALOG entries (cnt_t > 1: ~6 %) have anything to add, the rest
            // stay out of the probes (the masks over the sources are still built from all their entries)
#pragma unroll
            for (int rr = 0; rr < S6_RPW; ++rr)
#pragma unroll
                for (int b = 0; b < S6_B; ++b) if ((v_s[rr][b] >> 16) <= 1u) ph_t[rr][b] = -1;       // (the targets' masks are not built again)
            direction(std::false_type{}, ph_s, lo_s, hi_s, ph_t, v_s, lo_t, hi_t);                   // (v_s: both sides' counts, packed)
        } else if constexpr (!PACKED) direction(std::false_type{}, ph_s, lo_s, hi_s, ph_t, v_t, lo_t, hi_t);      // the other way round
    }
    // finish: 4,096 pairs, 8 per thread; consecutive lanes run along the output's contiguous direction
#pragma unroll 4
    for (int q = 0; q < S6_T * S6_T / (64 * S6_WAVES); ++q) {
        const int idx = tid + 64 * S6_WAVES * q;
        const int fast = idx & 63, slow = idx >> 6;
        const int ls = condensed ? slow : fast, lt = condensed ? fast : slow;
        const int s = g_s[ls], t = g_t[lt];
        if (s < 0 || t < 0 || s >= t) continue;
        const uint32_t cons = acc[ls * S6_LD + lt];
        if constexpr (COUNT) {                                                       // metrics.py:45-53 (gcs), 75-80 (jc)
            out[pc_out_index(d, sh, s, t, k0 + lt, condensed)] = pc_set_value<MODE == S6_GCS ? PC_GCS : PC_JC>((int)cons, (int)(tot_s[ls] + tot_t[lt]), as_distance);
            continue;
        }
        double sim = 0.0;
        if (cons) sim = (double)cons / (double)(tot_s[ls] + tot_t[lt]);               // metrics.py:104-110 (pocp), 149-152 (af)
        out[pc_out_index(d, sh, s, t, k0 + lt, condensed)] = pc_finish(sim, as_distance);
    }
    __syncthreads();                                                                // the next tile clears acc and rewrites g_s, g_t
    }
}

__global__ void k_pair_entries(const int32_t* __restrict__ pham, const int32_t* __restrict__ len, const int32_t* __restrict__ cnt,
                               uint2* __restrict__ pair_len, uint2* __restrict__ pair_cnt, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) { pair_len[e] = make_uint2((uint32_t)pham[e], (uint32_t)len[e]); pair_cnt[e] = make_uint2((uint32_t)pham[e], (uint32_t)cnt[e]); }
}
int pc_launch_pair_entries(const int32_t* pham, const int32_t* len, const int32_t* cnt, uint2* pair_len, uint2* pair_cnt, int64_t n, hipStream_t st) {
    if (n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_pair_entries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pham, len, cnt, pair_len, pair_cnt, n);
    if (hipGetLastError() != hipSuccess) { pc_set_error("k_pair_entries launch failed"); return PC_ERR_HIP; }
    return PC_OK;
}

// A genome's entries of phams with at least two holders, dense ids, at the start of its own slot [ent_off[g], ent_off[g+1]) of the
// sp_* arrays; sp_rank[g][w] = first of them at or after dense word w; sp_end[g] = their end.  One WAVE per genome: 64 entries per
// step, kept ones compacted by ballot; then every lane finds the rank of its share of the words by bisection of the compact ids
// (one thread per genome walked ~100 entries and W2 words one after the other: 0.15 ms of a 1.9-ms upload at N = 2,000).
__global__ __launch_bounds__(256) void k_sp_build(int N, const uint32_t* __restrict__ ent_off, const int32_t* __restrict__ pham, const int32_t* __restrict__ len,
                                                  const int32_t* __restrict__ cnt, const int32_t* __restrict__ dense, int W2, int32_t* __restrict__ sp_pham,
                                                  uint2* __restrict__ sp_len, uint2* __restrict__ sp_cnt, uint32_t* __restrict__ sp_rank, uint32_t* __restrict__ sp_end) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= N) return;
    const uint32_t e0 = ent_off[g], e1 = ent_off[g + 1];
    uint32_t at = e0;
    for (uint32_t base = e0; base < e1; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        int id = -1, l = 0, c2 = 0;
        if (e < e1) { id = dense[pham[e]]; l = len[e]; c2 = cnt[e]; }
        const unsigned long long keep = __ballot(id >= 0);
        if (id >= 0) {
            const uint32_t to = at + (uint32_t)__popcll(keep & ((1ULL << lane) - 1ULL));
            sp_pham[to] = id; sp_len[to] = make_uint2((uint32_t)id, (uint32_t)l); sp_cnt[to] = make_uint2((uint32_t)id, (uint32_t)c2);
        }
        at += (uint32_t)__popcll(keep);
    }
    if (lane == 0) sp_end[g] = at;
    __threadfence();                                                                // the wave's own stores are read back below (loads at agent scope: not from a stale L1 line)
    uint32_t* rank = sp_rank + (int64_t)g * W2;
    for (int w = lane; w < W2; w += 64) {                                           // first kept entry with id >= 64 w
        uint32_t lo = e0, hi = at;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (__hip_atomic_load(&sp_pham[mid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 64 * w) lo = mid + 1; else hi = mid; }
        rank[w] = lo;
    }
}
int pc_launch_sp_build(int N, const uint32_t* ent_off, const int32_t* pham, const int32_t* len, const int32_t* cnt, const int32_t* dense, int W2,
                       int32_t* sp_pham, uint2* sp_len, uint2* sp_cnt, uint32_t* sp_rank, uint32_t* sp_end, hipStream_t st) {
    if (N <= 0) return PC_OK;
    hipLaunchKernelGGL(k_sp_build, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, N, ent_off, pham, len, cnt, dense, W2, sp_pham, sp_len, sp_cnt, sp_rank, sp_end);
    if (hipGetLastError() != hipSuccess) { pc_set_error("k_sp_build launch failed"); return PC_ERR_HIP; }
    return PC_OK;
}

int pc_launch_sparse64(int mode, const PcDev& d, const PcShard& sh, double* out, int as_distance, int condensed, hipStream_t st, pc_set_shape* shape_out) {
    pc_set_shape shp;
    pc_set_shape_of(K_SPARSE64, pc_metric_of_mode(mode), d.N, sh.nown, d.Wb, d.sp_W, d.n_cu, 0, pc_set_knobs_env(), &shp);
    if (shape_out) *shape_out = shp;
    if (sh.nown <= 0 || d.N <= 1) return PC_OK;
    const int CH = shp.chunk;
    const size_t lds = (size_t)shp.lds;
    const unsigned n_units = (unsigned)shp.units;
    dim3 grid((unsigned)shp.grid), block(64 * S6_WAVES);
    // (up to 78 KB of dynamic LDS: HIP on this hardware needs no opt-in above 64 KB -- the K4 launches take up to 160 KB the same way)
    const bool known = pc_dispatch<S6_GCS, S6_JC, PCW_POCP, PCW_AF>(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (shp.batches == 1) hipLaunchKernelGGL((k_sparse_tile64<M, 1>), grid, block, lds, st, d, sh, out, as_distance, condensed, CH, n_units);
        else hipLaunchKernelGGL((k_sparse_tile64<M, 2>), grid, block, lds, st, d, sh, out, as_distance, condensed, CH, n_units);
    });
    if (!known) { pc_set_error("pc_launch_sparse64: bad mode %d", mode); return PC_ERR_ARG; }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_sparse_tile64 launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
