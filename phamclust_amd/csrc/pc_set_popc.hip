// pc_set_popc.hip -- gcs / jc / pocp as bitset-intersection popcounts over tiles of genome pairs: the 64x64 tile kernel, its word-split
// 32x32 twin for small matrices, the epilogue table both look their values up in, and pocp's paralog probe.
//
// Reference semantics restated here (metrics.py of the reference):
//   metrics.py:26-53, 56-80   gcs / jc closed forms on |B[s] & B[t]|   (pc_set_value, pc_pairs.h)
//   metrics.py:83-115         pocp: conserved gene count over the shared phams = 2 |S n T| + the paralogs' excess
//
// K1+K3: gcs / jc.  shared = popcount(B[s] & B[t]); fp64 epilogue.  One 256-thread workgroup
// per 64x64 tile of pairs, a 4x4 register tile of pairs per thread: per bitmap word a thread
// reads 4 source-row words and 4 target-row words from LDS (broadcast / conflict-free with
// the odd row stride) and does 16 AND+popcount pairs.  Lanes 0..15 of a 16-lane group hold
// consecutive t, so each store instruction writes 128-byte runs of the condensed output.
// The epilogue value depends only on the two small integers (shared, nph_s + nph_t), so it is
// looked up in a table built once per fill by k_set_lut (exactly the same fp64 code path:
// division, 1 - x, round(., 6)); without a table (huge genomes) it is computed in place.
// The bitmap is staged chunk by chunk in LDS, row stride padded to an odd number of u64 so that ds_read_b64 by lanes of distinct
// rows is conflict-free.  HBM/LDS-bound integer work: no MFMA.
#include "pc_pairs.h"

#define PWCH 32        // bitmap words staged per chunk

// pocp on the popcount kernels (r03).  conserved(s, t) = sum over shared phams of cnt_s + cnt_t = 2 |S n T| + the EXCESS
// counts (cnt - 1) of the shared phams that are paralogs in s or in t -- and only ~6 % of a genome's entries are
// paralogs.  So the kernel counts |S n T| exactly as for jc and, per staged chunk of bitmap words, lets the few paralog
// entries (pham, cnt - 1; ascending pham, so a cursor per row walks them chunk by chunk) of the rows it holds test their
// bit in the opposite rows (LDS) and add their excess.  ONLY >= 0: probe register-tile row ONLY alone (the word-split
// kernel gives each wave one row of each side, so that the four waves do not walk the same lists four times).
// (Staging the tile's lists in LDS first -- 12 packed entries per row, spill path for longer ones -- was built and measured
// slower: N = 20,000 4.54 against 4.29 ms; what costs is the divergence of 16 different rows per wave, not the list reads.)
struct PcParaRow { uint32_t cur, end; };
template <int ROWSTEP, int LDW, int ONLY>
__device__ __forceinline__ void pc_paralog_probe(const PcDev& d, PcParaRow (&st)[4], const uint64_t (*other)[LDW], int other0, int w0, int wn,
                                                 int (&ex)[4][4], bool rows_are_first_index) {
    const int p_end = (w0 + wn) * 64;
    // the four opposite rows as arrays of 32-bit halves: a test is one ds_read_b32 + bit extract + multiply-add
    const uint32_t* half[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) half[j] = (const uint32_t*)&other[other0 + ROWSTEP * j][0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (ONLY >= 0 && i != ONLY) continue;
        while (st[i].cur < st[i].end) {
            const int p = d.para_pham[st[i].cur];
            if (p >= p_end) break;
            const int e = d.para_ex[st[i].cur];
            ++st[i].cur;
            const int h = ((p >> 5) - 2 * w0), bit = p & 31;       // which 32-bit half of the staged chunk, which bit of it
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int hit = (int)((half[j][h] >> bit) & 1u);
                if (rows_are_first_index) ex[i][j] += e * hit; else ex[j][i] += e * hit;
            }
        }
    }
}

// ---- what the two popcount kernels share -------------------------------------------

// Staging through registers: thread (r0 = tid >> 5, w = tid & 31) moves word w of rows r0 + 8p (p < NP = tile edge / 8) of both sides of
// the tile; the next chunk's words are fetched into registers while the current chunk is being counted.
template <int NP>
struct PcPopcStage {
    const uint64_t* ps[NP]; const uint64_t* pt[NP];             // the rows' bitmap words, NULL: no such row
    uint64_t vs[NP], vt[NP];
    __device__ __forceinline__ void rows(const PcDev& d, const PcShard& sh, int s0, int k0) {
        const int r0 = threadIdx.x >> 5;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int s = s0 + r0 + 8 * p, k = k0 + r0 + 8 * p;
            ps[p] = s < d.N ? d.bitmap + (int64_t)s * d.Wstride : nullptr;
            pt[p] = k < sh.nown ? d.bitmap + (int64_t)pc_owned(sh, k) * d.Wstride : nullptr;
        }
    }
    __device__ __forceinline__ void fetch(const PcDev& d, int w0) {
        const int w = w0 + (threadIdx.x & 31);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            vs[p] = (ps[p] && w < d.Wb) ? ps[p][w] : 0ULL;
            vt[p] = (pt[p] && w < d.Wb) ? pt[p][w] : 0ULL;
        }
    }
    __device__ __forceinline__ void store(uint64_t (*rs)[PWCH + 1], uint64_t (*rt)[PWCH + 1]) const {
        const int r0 = threadIdx.x >> 5, wl = threadIdx.x & 31;
#pragma unroll
        for (int p = 0; p < NP; ++p) { rs[r0 + 8 * p][wl] = vs[p]; rt[r0 + 8 * p][wl] = vt[p]; }
    }
};

// genome of tile row `local` of the a side (the slow index: the tile's s rows under condensed output, its t rows otherwise) or the b
// side; -1: the row lies outside the matrix
__device__ __forceinline__ int pc_popc_genome(const PcDev& d, const PcShard& sh, int condensed, int s0, int k0, bool a_side, int local) {
    if (a_side == (condensed != 0)) return s0 + local < d.N ? s0 + local : -1;                 // an s row
    return k0 + local < sh.nown ? pc_owned(sh, k0 + local) : -1;                               // a t row
}

// acc += popcount(x): two v_bcnt_u32_b32, each adding into the running count (left to itself the compiler counts into a temporary
// and spends a third instruction on the add)
__device__ __forceinline__ void pc_popc_add(int& acc, uint64_t x) {
    asm("v_bcnt_u32_b32 %0, %1, %0\n\tv_bcnt_u32_b32 %0, %2, %0" : "+v"(acc) : "v"((uint32_t)x), "v"((uint32_t)(x >> 32)));
}

template <int METRIC>
__global__ void k_set_lut(double* __restrict__ lut, int sh_dim, int tot_dim, int as_distance) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= sh_dim * tot_dim) return;
    const int tot = i / sh_dim, shared = i - tot * sh_dim;
    // entries with shared > tot/2 (gcs) or shared > tot - shared (jc), conserved > total (pocp) never occur; keep them finite
    const bool possible = METRIC == PC_POCP ? shared <= tot : 2 * shared <= tot;
    lut[i] = possible ? pc_set_value<METRIC>(shared, tot, as_distance) : 0.0;
}


// (the pocp instance takes 166 registers and runs three waves per SIMD where gcs / jc run four; forcing four with
// amdgpu_waves_per_eu spills 40 dwords and costs 20 %: N = 20,000 4.02 -> 4.88 ms)
template <int METRIC>
__global__ __launch_bounds__(256) void k_set_popc(PcDev d, PcShard sh, int as_distance, double* __restrict__ out, int condensed,
                                                   const double* __restrict__ lut, int sh_dim) {
    constexpr int PT = 64;
    __shared__ uint64_t rs[PT][PWCH + 1];
    __shared__ uint64_t rt[PT][PWCH + 1];
    int tile_x, tile_y;
    if (!pc_tile_of_block((d.N + PT - 1) / PT, (sh.nown + PT - 1) / PT, tile_x, tile_y)) return;
    const int s0 = tile_x * PT, k0 = tile_y * PT;
    const int klast = min(k0 + PT, sh.nown) - 1;
    if (s0 >= pc_owned(sh, klast)) return;                   // tile entirely on/below the diagonal
    // 256 threads = 16 (fx) x 16 (fy), a 4x4 register tile of pairs each: per bitmap word a thread reads 4 + 4 row words
    // from LDS for 16 AND+popcount pairs (0.5 LDS reads per pair-word: the loop is VALU-bound -- v_and at 2 clocks and
    // v_bcnt at 4 per wave64, profiles/valu_issue_rate.json -- not LDS-bound).  fx runs along the output's contiguous
    // direction: t (condensed) or s (shard-local), so each store instruction writes 128-byte runs.
    const int fx = threadIdx.x & 15, fy = threadIdx.x >> 4;
    int acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    PcPopcStage<PT / 8> stage;
    stage.rows(d, sh, s0, k0);
    // the rows a thread reads: the slow index takes the tile's s rows under condensed output, its t rows otherwise
    uint64_t (*ra)[PWCH + 1] = condensed ? rs : rt;
    uint64_t (*rb)[PWCH + 1] = condensed ? rt : rs;
    // pocp: the paralog lists of my 4 + 4 rows (rows outside the matrix have empty lists)
    // The b side is probed under TRANSPOSED ownership: this thread walks the lists of b-rows fy + 16 i (the wave's lanes share
    // fy in groups of 16, so a wave sees 4 distinct lists per i, as on the a side -- with its own b-rows fx + 16 i it would see
    // 16, and the loop runs as long as the longest) against a-rows fx + 16 j, and the sums meet their owners through LDS at the end.
    int ex[4][4], ex2[4][4];
    PcParaRow st_a[4], st_b[4];
    if (METRIC == PC_POCP) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ex[i][j] = ex2[i][j] = 0;
            const int ga = pc_popc_genome(d, sh, condensed, s0, k0, true, fy + 16 * i), gb = pc_popc_genome(d, sh, condensed, s0, k0, false, fy + 16 * i);
            st_a[i].cur = st_a[i].end = st_b[i].cur = st_b[i].end = 0;
            if (ga >= 0) { st_a[i].cur = d.para_off[ga]; st_a[i].end = d.para_off[ga + 1]; }
            if (gb >= 0) { st_b[i].cur = d.para_off[gb]; st_b[i].end = d.para_off[gb + 1]; }
        }
    }
    stage.fetch(d, 0);
    for (int w0 = 0; w0 < d.Wb; w0 += PWCH) {
        const int wn = min(PWCH, d.Wb - w0);
        if (w0) __syncthreads();
        stage.store(rs, rt);
        __syncthreads();
        if (w0 + PWCH < d.Wb) stage.fetch(d, w0 + PWCH);
        if (METRIC == PC_POCP) {
            pc_paralog_probe<16, PWCH + 1, -1>(d, st_a, rb, fx, w0, wn, ex, true);
            pc_paralog_probe<16, PWCH + 1, -1>(d, st_b, ra, fx, w0, wn, ex2, true);        // ex2[i][j]: b-row fy + 16 i, a-row fx + 16 j
        }
        for (int w = 0; w < wn; ++w) {
            uint64_t a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = ra[fy + 16 * i][w];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = rb[fx + 16 * j][w];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) pc_popc_add(acc[i][j], a[i] & b[j]);
        }
    }
    if (METRIC == PC_POCP) {                                         // b-side sums -> the threads that own the pairs (the staging rows are free now)
        __syncthreads();
        int* xt = (int*)&rs[0][0];                                   // [64 b-rows][65]  (16,640 of rs's 16,896 bytes)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) xt[(fy + 16 * i) * 65 + fx + 16 * j] = ex2[i][j];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) ex[i][j] += xt[(fx + 16 * j) * 65 + fy + 16 * i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ls = condensed ? fy + 16 * i : fx + 16 * j;
            const int lt = condensed ? fx + 16 * j : fy + 16 * i;
            const int s = s0 + ls, k = k0 + lt;
            if (s >= d.N || k >= sh.nown) continue;
            const int t = pc_owned(sh, k);
            if (s >= t) continue;
            const int shared = METRIC == PC_POCP ? 2 * acc[i][j] + ex[i][j] : acc[i][j];
            const int tot = METRIC == PC_POCP ? d.ngen[s] + d.ngen[t] : d.nph[s] + d.nph[t];
            const double v = lut ? lut[tot * sh_dim + shared] : pc_set_value<METRIC>(shared, tot, as_distance);
            out[pc_out_index(d, sh, s, t, k, condensed)] = v;
        }
    }
}

// The same for SMALL matrices: 32x32-pair tiles, and the four waves of a workgroup split the bitmap WORDS of the tile
// between them (wave v counts words v, v+4, ... of every chunk for all 32x32 pairs, 4x4 per lane), then add their partial
// counts through LDS and each finishes a quarter of the pairs.  At N = 2,000 (BASELINE configs[1]) the 64x64 kernel is 528
// live workgroups of ~11 us per wave on 256 CUs: two waves on most SIMDs, three on some, and the kernel lasts as long as
// the three (51 us against a 16 us popcount floor; counting alone 32 us, `tools/popc_experiment.sh`).  Here a wave carries
// a quarter of that, so 8,064 of them deal out evenly, and the ~8 waves per SIMD hide each other's LDS and staging waits.
// The staging buffers double as the partial-sum array once the last chunk has been counted.
// (Tried on top: wave-PRIVATE staging -- each wave loads the 20 words it will count for all 64 rows in one burst, no workgroup
// barrier before the final reduction -- 43 KB of LDS instead of 17: N = 2,000 36 -> 43 us, N = 5,000 166 -> 210: the nine
// resident workgroups per CU hide more than the barriers cost.)
template <int METRIC>
__global__ __launch_bounds__(256) void k_set_popc_ksplit(PcDev d, PcShard sh, int as_distance, double* __restrict__ out, int condensed,
                                                          const double* __restrict__ lut, int sh_dim) {
    constexpr int PT = 32;
    __shared__ uint64_t lds[2 * PT * (PWCH + 1)];                   // rs, rt; later int part[4][16][64] (16,384 of its 16,896 bytes)
    uint64_t (*rs)[PWCH + 1] = (uint64_t (*)[PWCH + 1])lds;
    uint64_t (*rt)[PWCH + 1] = (uint64_t (*)[PWCH + 1])(lds + PT * (PWCH + 1));
    int tile_x, tile_y;
    if (!pc_tile_of_block((d.N + PT - 1) / PT, (sh.nown + PT - 1) / PT, tile_x, tile_y)) return;
    const int s0 = tile_x * PT, k0 = tile_y * PT;
    const int klast = min(k0 + PT, sh.nown) - 1;
    if (s0 >= pc_owned(sh, klast)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fx = lane & 7, fy = lane >> 3;
    // the pairs this lane FINISHES: register-tile row `wave`, columns 0..3; their nph are fetched now, off the critical path
    int fin_s[4], fin_k[4], fin_t[4], fin_tot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ls = condensed ? fy + 8 * wave : fx + 8 * j, lt = condensed ? fx + 8 * j : fy + 8 * wave;
        fin_s[j] = s0 + ls; fin_k[j] = k0 + lt;
        const bool ok = fin_s[j] < d.N && fin_k[j] < sh.nown;
        fin_t[j] = ok ? pc_owned(sh, fin_k[j]) : 0;
        fin_tot[j] = !(ok && fin_s[j] < fin_t[j]) ? -1                                          // -1: no such pair
                     : METRIC == PC_POCP ? d.ngen[fin_s[j]] + d.ngen[fin_t[j]] : d.nph[fin_s[j]] + d.nph[fin_t[j]];
    }
    int acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    PcPopcStage<PT / 8> stage;
    stage.rows(d, sh, s0, k0);
    uint64_t (*ra)[PWCH + 1] = condensed ? rs : rt;
    uint64_t (*rb)[PWCH + 1] = condensed ? rt : rs;
    // pocp: wave v probes register-tile row v of each side (all words of every chunk); the partial sums meet in LDS below
    int ex[4][4];
    PcParaRow st_a[4], st_b[4];
    if (METRIC == PC_POCP) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ex[i][j] = 0;
            st_a[i].cur = st_a[i].end = st_b[i].cur = st_b[i].end = 0;
        }
        const int ga = pc_popc_genome(d, sh, condensed, s0, k0, true, fy + 8 * wave), gb = pc_popc_genome(d, sh, condensed, s0, k0, false, fx + 8 * wave);
        PcParaRow ra_st = {0, 0}, rb_st = {0, 0};
        if (ga >= 0) { ra_st.cur = d.para_off[ga]; ra_st.end = d.para_off[ga + 1]; }
        if (gb >= 0) { rb_st.cur = d.para_off[gb]; rb_st.end = d.para_off[gb + 1]; }
        if (wave == 0) { st_a[0] = ra_st; st_b[0] = rb_st; } else if (wave == 1) { st_a[1] = ra_st; st_b[1] = rb_st; }
        else if (wave == 2) { st_a[2] = ra_st; st_b[2] = rb_st; } else { st_a[3] = ra_st; st_b[3] = rb_st; }
    }
    stage.fetch(d, 0);
    for (int w0 = 0; w0 < d.Wb; w0 += PWCH) {
        const int wn = min(PWCH, d.Wb - w0);
        if (w0) __syncthreads();
        stage.store(rs, rt);
        __syncthreads();
        if (w0 + PWCH < d.Wb) stage.fetch(d, w0 + PWCH);
        if (METRIC == PC_POCP) {                                     // this wave's words of the chunk: wave, wave + 4, ...
            pc_paralog_probe<8, PWCH + 1, -1>(d, st_a, rb, fx, w0, wn, ex, true);      // (the other three rows' lists are empty)
            pc_paralog_probe<8, PWCH + 1, -1>(d, st_b, ra, fy, w0, wn, ex, false);
        }
#pragma unroll
        for (int q = 0; q < PWCH / 4; ++q) {
            const int w = wave + 4 * q;                              // wave-uniform
            if (w >= wn) break;
            uint64_t a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = ra[fy + 8 * i][w];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = rb[fx + 8 * j][w];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) pc_popc_add(acc[i][j], a[i] & b[j]);
        }
    }
    __syncthreads();                                                 // every wave is done with the staged words
    int* part = (int*)lds;                                           // [wave][i * 4 + j][lane]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(wave * 16 + i * 4 + j) * 64 + lane] = METRIC == PC_POCP ? 2 * acc[i][j] + ex[i][j] : acc[i][j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int shared = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) shared += part[(v * 16 + wave * 4 + j) * 64 + lane];
        if (fin_tot[j] < 0) continue;
        const double val = lut ? lut[fin_tot[j] * sh_dim + shared] : pc_set_value<METRIC>(shared, fin_tot[j], as_distance);
        out[pc_out_index(d, sh, fin_s[j], fin_t[j], fin_k[j], condensed)] = val;
    }
}

int pc_launch_set_popc(const PcDev& d, const PcShard& sh, int metric, int as_distance, double* out, int condensed,
                       double* lut, bool build_lut, int top, hipStream_t st, pc_set_shape* shape_out) {
    pc_set_shape shp;
    pc_set_shape_of(K_POPC, metric, d.N, sh.nown, d.Wb, d.sp_W, d.n_cu, top, pc_set_knobs_env(), &shp);
    if (!lut) shp.table = 0;                                                               // (the caller could not hold one)
    if (shape_out) *shape_out = shp;
    if (sh.nown <= 0 || d.N <= 1) return PC_OK;
    int sh_dim = 0, tot_dim = 0;
    (void)pc_set_table_dims(metric, top, &sh_dim, &tot_dim);
    const dim3 grid((unsigned)shp.grid);
    const bool known = pc_dispatch<PC_GCS, PC_JC, PC_POCP>(metric, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (lut && build_lut) hipLaunchKernelGGL(k_set_lut<M>, dim3((sh_dim * tot_dim + 255) / 256), dim3(256), 0, st, lut, sh_dim, tot_dim, as_distance);
        if (shp.tile == 32) hipLaunchKernelGGL(k_set_popc_ksplit<M>, grid, dim3(256), 0, st, d, sh, as_distance, out, condensed, (const double*)lut, sh_dim);
        else hipLaunchKernelGGL(k_set_popc<M>, grid, dim3(256), 0, st, d, sh, as_distance, out, condensed, (const double*)lut, sh_dim);
    });
    if (!known) { pc_set_error("pc_launch_set_popc: bad metric %d", metric); return PC_ERR_ARG; }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_set_popc launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
