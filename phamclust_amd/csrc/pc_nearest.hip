// pc_nearest.hip -- the kernels of pc_fill_nearest: every genome's K best neighbours (K <= 64), merged slab by slab into K slots per
// genome that stay on the device for the length of the call, as parent[N] does for the components fill.
//   state   key[N][K] u64, nbr[N][K] i32, each row sorted best first.  The key is an order-preserving transform of the value's f64
//           bits (sign bit flipped for values >= 0, every bit for values < 0: unsigned order = f64 order), complemented on a
//           similarity fill, so that BETTER IS THE SMALLER KEY in both directions and the kernels have one code path; behind it the
//           genome index is compared, smaller first.  (key, index) is the total order of the header: the K smallest of it are the
//           result, whatever order the candidates arrive in.  Empty slots hold the worst sentinel (key ~0, index INT32_MAX); every
//           genome meets N - 1 >= K candidates in the course of a call, so none is left at the end.
//   k_nn_init    the sentinel
//   k_nn_rows    a slab of targets [t0, t1) holds for target t the values of (s, t), s < t, contiguously at lbase(t) + s with
//                lbase(t) = t(t-1)/2 - t0(t0-1)/2 (the slab's shard layout in closed form: its targets are consecutive).  One wave per
//                target: 64 lanes read 64 consecutive sources, 512 contiguous bytes.
//   k_nn_cols    source s takes the candidates (t, v), t in [max(s + 1, t0), t1).  For one t the values of 64 consecutive sources are
//                512 contiguous bytes: a workgroup owns a block of 64 sources and walks the targets in tiles of 64, each tile read
//                row by row (lanes across sources, one 512-byte run per target) into LDS as keys; then each of its four waves takes 16
//                of the sources, whose lists it keeps in registers across all the tiles, and reads a source's column of the tile
//                lanes across targets (row stride 65: no bank conflict).
//   k_nn_finish  val = the value behind each key
//   k_nn_merge   several devices, each with the lists of its own stretch of targets (pc_multi_fill_nearest): the lists of the other
//                devices, staged on the root as fkey / fnbr [n_foreign][N][K], go into the root's, one wave per genome.  A pair lies
//                in exactly one stretch (its target's), so no real entry occurs twice; a foreign list may end in worst sentinels (its
//                device need not have met K candidates of the genome), which are no candidates.
//   k_nn_qrows / k_nn_qcols   the two passes of pc_fill_rows_nearest over a ROWS slab (PcRowsSlab: f64[m][n], row r the values of query
//                genome rows[r] against every genome), which grow lists seeded from a stored result.  They are no flat passes -- a wave
//                or a workgroup owns whole rows or whole columns of the slab, not a run of its elements -- so they do not go through
//                pc_slab_pass.h; they take the PcRowsSlab as it is (adv_* unused).
//                k_nn_qrows: one wave per slab row, q = rows[r]: the candidates (v[r][g], g) for every g != q, other query genomes
//                included -- a query row lies in exactly one slab, so the list, begun empty, is complete after this one wave.
//                k_nn_qcols: a workgroup owns 64 consecutive genomes (columns) and walks the slab's rows in tiles of 64, staged as
//                keys into LDS (stride 65, one 512-byte run per row); each of its four waves holds 16 columns' lists in registers
//                and reads a column of the tile lanes across rows, exactly as k_nn_cols; the candidate's index is rows[row].  A
//                column that is itself a query genome is skipped whole (its list is k_nn_qrows'); rows >= m and columns >= n stage
//                the worst sentinel and are no candidates.  Nothing is read beyond m * n values.
//   k_nn_pair_entries / k_nn_run_starts / k_nn_pairs   pc_nearest_of_pairs: the same lists from a PAIR LIST instead of a slab (their section
//                below): a wave per genome over the sorted run of its pairs, through the same wave step.
// A genome's list lives one entry per lane of a wave (why K <= 64).  The K-th entry is "the bar": a ballot of `candidate beats the
// bar` finds the few candidates that matter (after the warm-up about K ln(n / K) per genome); each of them is inserted at the
// position popcount(ballot(entry comes before the candidate)), the lanes behind it taking their lower neighbour's entry.
// Who writes what: the list of genome g is written by exactly one wave per launch -- in k_nn_rows the wave of target g, in k_nn_cols
// the wave that owns source g; in k_nn_qrows the wave of query row g, in k_nn_qcols the wave that owns the old column g -- and the
// launches are ordered on the stream.  No atomics, no flags, nothing one workgroup waits for from another.  Nothing is read beyond Lp:
// an element lbase(t) + s is read only for s < t < t1, an element row * n + g of a rows slab only for row < m, g < n; loads are 8 bytes wide.
#include "pc_pairs.h"

#define NN_THREADS 256
#define NN_WAVES (NN_THREADS / 64)
#define NN_TILE 64                                     // targets and sources of a column-pass tile
#define NN_LD (NN_TILE + 1)                            // row stride of the tile in LDS (u64 elements)
#define NN_SRC_PER_WAVE (NN_TILE / NN_WAVES)           // 16 lists in a wave's registers
#define NN_WORST_KEY (~0ull)
#define NN_WORST_IDX 0x7fffffff

typedef unsigned long long nn_key;

// flip: 0 on a distance fill, ~0 on a similarity fill
__device__ __forceinline__ nn_key nn_key_of(double v, nn_key flip) {
    const nn_key u = (nn_key)__double_as_longlong(v);
    return (u ^ ((u >> 63) ? ~0ull : (1ull << 63))) ^ flip;
}
__device__ __forceinline__ double nn_value_of(nn_key k, nn_key flip) {
    const nn_key u = k ^ flip;
    return __longlong_as_double((long long)(u ^ ((u >> 63) ? (1ull << 63) : ~0ull)));
}
__device__ __forceinline__ bool nn_before(nn_key ka, int ia, nn_key kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

// lane `src` of x for the whole wave; src is wave-uniform (K - 1, or a bit position of a ballot): v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ int nn_lane(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ __forceinline__ nn_key nn_lane(nn_key x, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), src);
    return ((nn_key)hi << 32) | lo;
}
__device__ __forceinline__ nn_key nn_shfl_up1(nn_key x) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)x, 1), hi = (unsigned)__shfl_up((int)(unsigned)(x >> 32), 1);
    return ((nn_key)hi << 32) | lo;
}

// One wave's step over up to 64 candidates, one per lane ((ck, ci), have): those that beat the bar go into the list (ek, ei) that the
// wave holds one entry per lane (lanes >= K carry nothing that is ever read).  Wave-uniform control flow throughout.
__device__ __forceinline__ void nn_take(nn_key& ek, int& ei, nn_key ck, int ci, bool have, int K, int lane) {
    nn_key bk = nn_lane(ek, K - 1);
    int bi = nn_lane(ei, K - 1);
    unsigned long long m = __ballot(have && nn_before(ck, ci, bk, bi));
    while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const nn_key k = nn_lane(ck, j);
        const int i = nn_lane(ci, j);
        if (!nn_before(k, i, bk, bi)) continue;        // (an earlier candidate of this step raised the bar)
        // entries that come before the candidate are a prefix of the sorted list, and lane K - 1 (the bar) is not among them: pos < K
        const int pos = __popcll(__ballot(lane < K && nn_before(ek, ei, k, i)));
        const nn_key uk = nn_shfl_up1(ek);
        const int ui = __shfl_up(ei, 1);
        if (lane > pos) { ek = uk; ei = ui; }
        else if (lane == pos) { ek = k; ei = i; }
        bk = nn_lane(ek, K - 1);
        bi = nn_lane(ei, K - 1);
    }
}

__device__ __forceinline__ int64_t nn_pairs_below(int t) { return (int64_t)t * (t - 1) / 2; }

__global__ __launch_bounds__(256) void k_nn_init(nn_key* __restrict__ key, int32_t* __restrict__ nbr, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { key[i] = NN_WORST_KEY; nbr[i] = NN_WORST_IDX; }
}

// row pass: wave w of workgroup b takes target t0 + b * NN_WAVES + w
__global__ __launch_bounds__(NN_THREADS) void k_nn_rows(const double* __restrict__ vals, int t0, int t1, nn_key flip, int K,
                                                        nn_key* __restrict__ key, int32_t* __restrict__ nbr) {
    const int lane = threadIdx.x & 63;
    const int t = t0 + (int)blockIdx.x * NN_WAVES + (int)(threadIdx.x >> 6);
    if (t >= t1 || t == 0) return;                     // (the whole wave; genome 0 has no row part)
    const double* __restrict__ row = vals + (nn_pairs_below(t) - nn_pairs_below(t0));
    const size_t at = (size_t)t * K + lane;
    nn_key ek = NN_WORST_KEY; int ei = NN_WORST_IDX;
    if (lane < K) { ek = key[at]; ei = nbr[at]; }      // the list as the slabs before left it: the bar is tight from the second slab on
    for (int base = 0; base < t; base += 128) {        // two independent 512-byte loads in flight
        const int s0 = base + lane, s1 = base + 64 + lane;
        const bool h0 = s0 < t, h1 = s1 < t;
        const double v0 = h0 ? row[s0] : 0.0, v1 = h1 ? row[s1] : 0.0;
        nn_take(ek, ei, nn_key_of(v0, flip), s0, h0, K, lane);
        if (base + 64 < t) nn_take(ek, ei, nn_key_of(v1, flip), s1, h1, K, lane);
    }
    if (lane < K) { key[at] = ek; nbr[at] = ei; }
}

// column pass: workgroup b takes the sources [64 b, 64 b + 64) below t1 - 1 (genome t1 - 1 has no column part in this slab, genome
// N - 1 in none)
__global__ __launch_bounds__(NN_THREADS) void k_nn_cols(const double* __restrict__ vals, int t0, int t1, nn_key flip, int K,
                                                        nn_key* __restrict__ key, int32_t* __restrict__ nbr) {
    __shared__ nn_key tile[NN_TILE * NN_LD];           // [target of the tile][source of the block], 33,280 bytes
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sb = (int)blockIdx.x * NN_TILE;          // first source of the block
    const int s_end = t1 - 1;                          // sources of the slab: s < t1 - 1
    const int64_t below0 = nn_pairs_below(t0);
    nn_key lk[NN_SRC_PER_WAVE]; int li[NN_SRC_PER_WAVE];
#pragma unroll
    for (int q = 0; q < NN_SRC_PER_WAVE; ++q) {
        const int s = sb + wv * NN_SRC_PER_WAVE + q;
        lk[q] = NN_WORST_KEY; li[q] = NN_WORST_IDX;
        if (s < s_end && lane < K) { lk[q] = key[(size_t)s * K + lane]; li[q] = nbr[(size_t)s * K + lane]; }
    }
    // the block's first target: above its first source, inside the slab (sb < t1 - 1: the range is not empty)
    for (int tb = max(sb + 1, t0); tb < t1; tb += NN_TILE) {
        // stage: row r of the tile = target tb + r, lanes across the block's sources; only elements with s < t < t1 exist
#pragma unroll
        for (int i = 0; i < NN_TILE / NN_WAVES; ++i) {  // (sixteen independent 512-byte loads in flight per wave)
            const int r = wv + i * NN_WAVES, t = tb + r, s = sb + lane;
            nn_key k = NN_WORST_KEY;
            if (t < t1 && s < t) k = nn_key_of(vals[nn_pairs_below(t) - below0 + s], flip);
            tile[r * NN_LD + lane] = k;
        }
        __syncthreads();
        const int t = tb + lane;                       // this lane's candidate of every source of the wave
#pragma unroll
        for (int q = 0; q < NN_SRC_PER_WAVE; ++q) {
            const int c = wv * NN_SRC_PER_WAVE + q, s = sb + c;
            if (s >= s_end) break;                     // (wave-uniform; the ragged last block)
            nn_take(lk[q], li[q], tile[lane * NN_LD + c], t, t < t1 && t > s, K, lane);
        }
        __syncthreads();                               // the tile is rewritten by the next round
    }
#pragma unroll
    for (int q = 0; q < NN_SRC_PER_WAVE; ++q) {
        const int s = sb + wv * NN_SRC_PER_WAVE + q;
        if (s < s_end && lane < K) { key[(size_t)s * K + lane] = lk[q]; nbr[(size_t)s * K + lane] = li[q]; }
    }
}

// query-row pass of a rows slab: wave w of workgroup b takes slab row b * NN_WAVES + w
__global__ __launch_bounds__(NN_THREADS) void k_nn_qrows(const double* __restrict__ vals, PcRowsSlab dom, nn_key flip, int K,
                                                         nn_key* __restrict__ key, int32_t* __restrict__ nbr) {
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * NN_WAVES + (int)(threadIdx.x >> 6);
    if (r >= dom.m) return;                            // (the whole wave)
    const int n = dom.n, q = dom.rows[r];
    const double* __restrict__ row = vals + (size_t)r * n;
    nn_key ek = NN_WORST_KEY; int ei = NN_WORST_IDX;   // a query genome's list begins empty: all its n - 1 >= K candidates are in this row
    for (int base = 0; base < n; base += 128) {        // two independent 512-byte loads in flight
        const int g0 = base + lane, g1 = base + 64 + lane;
        const bool i0 = g0 < n, i1 = g1 < n;
        const double v0 = i0 ? row[g0] : 0.0, v1 = i1 ? row[g1] : 0.0;
        nn_take(ek, ei, nn_key_of(v0, flip), g0, i0 && g0 != q, K, lane);
        if (base + 64 < n) nn_take(ek, ei, nn_key_of(v1, flip), g1, i1 && g1 != q, K, lane);
    }
    const size_t at = (size_t)q * K + lane;
    if (lane < K) { key[at] = ek; nbr[at] = ei; }
}

// old-column pass of a rows slab: workgroup b takes the genomes [64 b, 64 b + 64) as columns
__global__ __launch_bounds__(NN_THREADS) void k_nn_qcols(const double* __restrict__ vals, PcRowsSlab dom, nn_key flip, int K,
                                                         nn_key* __restrict__ key, int32_t* __restrict__ nbr) {
    __shared__ nn_key tile[NN_TILE * NN_LD];           // [row of the tile][column of the block], 33,280 bytes
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = dom.m, n = dom.n;
    const int cb = (int)blockIdx.x * NN_TILE;          // first column of the block
    nn_key lk[NN_SRC_PER_WAVE]; int li[NN_SRC_PER_WAVE];
    unsigned skip = 0;                                 // bit q: the wave's column q is beyond n or a query genome (wave-uniform)
#pragma unroll
    for (int q = 0; q < NN_SRC_PER_WAVE; ++q) {
        const int g = cb + wv * NN_SRC_PER_WAVE + q;
        const bool live = g < n && !dom.is_query[g];
        if (!live) skip |= 1u << q;
        lk[q] = NN_WORST_KEY; li[q] = NN_WORST_IDX;
        if (live && lane < K) { lk[q] = key[(size_t)g * K + lane]; li[q] = nbr[(size_t)g * K + lane]; }
    }
    skip = (unsigned)__builtin_amdgcn_readfirstlane((int)skip);
    for (int rb = 0; rb < m; rb += NN_TILE) {
        // stage: row i of the tile = slab row rb + i, lanes across the block's columns; only elements with row < m, column < n exist
#pragma unroll
        for (int i = 0; i < NN_TILE / NN_WAVES; ++i) {  // (sixteen independent 512-byte loads in flight per wave)
            const int tr = wv + i * NN_WAVES, row = rb + tr, g = cb + lane;
            nn_key k = NN_WORST_KEY;
            if (row < m && g < n) k = nn_key_of(vals[(size_t)row * n + g], flip);
            tile[tr * NN_LD + lane] = k;
        }
        __syncthreads();
        const int row = rb + lane;                     // this lane's candidate of every column of the wave: the query genome of its row
        const bool have = row < m;
        const int ci = have ? dom.rows[row] : NN_WORST_IDX;
#pragma unroll
        for (int q = 0; q < NN_SRC_PER_WAVE; ++q) {
            if ((skip >> q) & 1u) continue;            // (wave-uniform)
            nn_take(lk[q], li[q], tile[lane * NN_LD + wv * NN_SRC_PER_WAVE + q], ci, have, K, lane);
        }
        __syncthreads();                               // the tile is rewritten by the next round
    }
#pragma unroll
    for (int q = 0; q < NN_SRC_PER_WAVE; ++q) {
        const int g = cb + wv * NN_SRC_PER_WAVE + q;
        if (!((skip >> q) & 1u) && lane < K) { key[(size_t)g * K + lane] = lk[q]; nbr[(size_t)g * K + lane] = li[q]; }
    }
}

__global__ __launch_bounds__(256) void k_nn_finish(const nn_key* __restrict__ key, double* __restrict__ val, int64_t n, nn_key flip) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) val[i] = nn_value_of(key[i], flip);
}

// merge pass: wave w of workgroup b takes genome b * NN_WAVES + w, as k_nn_rows deals targets.  The list of g is written by this wave
// alone; nothing is read beyond n_foreign * N * K entries.
__global__ __launch_bounds__(NN_THREADS) void k_nn_merge(nn_key* __restrict__ key, int32_t* __restrict__ nbr, const nn_key* __restrict__ fkey,
                                                         const int32_t* __restrict__ fnbr, int n_foreign, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int g = (int)blockIdx.x * NN_WAVES + (int)(threadIdx.x >> 6);
    if (g >= N) return;                                // (the whole wave)
    const size_t at = (size_t)g * K + lane;
    nn_key ek = NN_WORST_KEY; int ei = NN_WORST_IDX;
    if (lane < K) { ek = key[at]; ei = nbr[at]; }
    for (int f = 0; f < n_foreign; ++f) {
        const size_t fat = ((size_t)f * N + g) * K + lane;
        nn_key fk = NN_WORST_KEY; int fi = NN_WORST_IDX;
        if (lane < K) { fk = fkey[fat]; fi = fnbr[fat]; }
        nn_take(ek, ei, fk, fi, lane < K && fi != NN_WORST_IDX, K, lane);
    }
    if (lane < K) { key[at] = ek; nbr[at] = ei; }
}

// ---- pc_nearest_of_pairs: the lists of a PAIR LIST (src / tgt / val [L], any order, no pair twice, no diagonal), every pair a
// candidate of both its ends.
//   k_nn_pair_entries  the 2 L directed entries: entry d < L is pair d seen from its source (owner src[d], other tgt[d]), entry L + d
//                      the same pair from its target; key = owner << 32 | other, value = the pair's position d
//   (pc_sort_pairs by the key: an owner's entries become one run)
//   k_nn_run_starts    start[g], g = 0 .. N: the first sorted entry whose owner is >= g, by binary search (start[N] = 2 L); owners
//                      without a pair get an empty run
//   k_nn_pairs         one wave per owner walks its run 64 entries a step through nn_take -- the candidate is (key of val[position],
//                      other) -- and writes the list, count[g] = the run's length, and the padding behind it
// The run is in index order within equal values already; nn_take compares (key, index) all the same.  The list of g is written by the
// wave of g alone; nothing is read beyond 2 L entries or beyond val[L].
#define NN_PAD_IDX (-1)
#define NN_QUIET_NAN 0x7ff8000000000000ll

__global__ __launch_bounds__(256) void k_nn_pair_entries(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt, nn_key* __restrict__ dkey,
                                                         uint32_t* __restrict__ dpos, int64_t L) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= 2 * L) return;
    const int64_t p = d < L ? d : d - L;
    const uint32_t s = (uint32_t)src[p], t = (uint32_t)tgt[p];
    dkey[d] = d < L ? ((nn_key)s << 32) | t : ((nn_key)t << 32) | s;
    dpos[d] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void k_nn_run_starts(const nn_key* __restrict__ skey, int64_t n, int N, uint32_t* __restrict__ start) {
    const int g = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (g > N) return;
    const nn_key bound = (nn_key)(uint32_t)g << 32;
    int64_t lo = 0, hi = n;                            // the first entry with skey >= bound lies in [lo, hi]
    while (lo < hi) { const int64_t mid = lo + (hi - lo) / 2; if (skey[mid] < bound) lo = mid + 1; else hi = mid; }
    start[g] = (uint32_t)lo;
}

// wave w of workgroup b takes owner b * NN_WAVES + w
__global__ __launch_bounds__(NN_THREADS) void k_nn_pairs(const nn_key* __restrict__ skey, const uint32_t* __restrict__ spos, const double* __restrict__ val,
                                                         const uint32_t* __restrict__ start, int N, nn_key flip, int K, nn_key* __restrict__ key,
                                                         int32_t* __restrict__ nbr, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int g = (int)blockIdx.x * NN_WAVES + (int)(threadIdx.x >> 6);
    if (g >= N) return;                                // (the whole wave)
    const uint32_t d0 = start[g], d1 = start[g + 1];
    nn_key ek = NN_WORST_KEY; int ei = NN_WORST_IDX;
    for (uint32_t base = d0; base < d1; base += 64) {  // (2 L <= 2^31: base + 64 does not wrap)
        const uint32_t d = base + (uint32_t)lane;
        const bool have = d < d1;
        nn_key ck = NN_WORST_KEY; int ci = NN_WORST_IDX;
        if (have) { ci = (int)(uint32_t)skey[d]; ck = nn_key_of(val[spos[d]], flip); }
        nn_take(ek, ei, ck, ci, have, K, lane);
    }
    const uint32_t n = d1 - d0;
    if (lane == 0) count[g] = (int32_t)n;
    if (lane < K) {
        const bool pad = (uint32_t)lane >= n;
        key[(size_t)g * K + lane] = pad ? nn_key_of(__longlong_as_double(NN_QUIET_NAN), flip) : ek;
        nbr[(size_t)g * K + lane] = pad ? NN_PAD_IDX : ei;
    }
}

static int nn_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("%s launch: %s", what, hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

int pc_launch_nn_init(unsigned long long* key, int32_t* nbr, int64_t n, hipStream_t st) {
    if (n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_nn_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, key, nbr, n);
    return nn_check("k_nn_init");
}

// vals: the filled slab of the targets [t0, t1), f64[Lp] with Lp = t1(t1-1)/2 - t0(t0-1)/2; key / nbr: [N][K], N >= t1, 1 <= K <= 64
int pc_launch_nn_select(const double* vals, int64_t Lp, int t0, int t1, int as_distance, int K, unsigned long long* key, int32_t* nbr, hipStream_t st) {
    if (K < 1 || K > 64 || t0 < 0 || t1 <= t0 || Lp != (int64_t)t1 * (t1 - 1) / 2 - (int64_t)t0 * (t0 - 1) / 2) {
        pc_set_error("pc_launch_nn_select: targets [%d, %d) with %lld pairs, K = %d", t0, t1, (long long)Lp, K);
        return PC_ERR_ARG;
    }
    if (Lp == 0) return PC_OK;
    const nn_key flip = as_distance ? 0ull : ~0ull;
    hipLaunchKernelGGL(k_nn_rows, dim3((unsigned)((t1 - t0 + NN_WAVES - 1) / NN_WAVES)), dim3(NN_THREADS), 0, st, vals, t0, t1, flip, K, key, nbr);
    int rc = nn_check("k_nn_rows");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_nn_cols, dim3((unsigned)((t1 - 1 + NN_TILE - 1) / NN_TILE)), dim3(NN_THREADS), 0, st, vals, t0, t1, flip, K, key, nbr);   // (Lp > 0: t1 >= 2)
    return nn_check("k_nn_cols");
}

// vals: one filled slab of a rows slab fill, f64[dom.m][dom.n] (Lp = m * n); key / nbr: [n][K], 1 <= K <= min(64, n - 1).  The lists
// of the slab's query genomes are written whole; those of the other genomes take the slab's rows as candidates.
int pc_launch_nn_select_rows(const double* vals, int64_t Lp, const PcRowsSlab& dom, int as_distance, int K, unsigned long long* key, int32_t* nbr,
                             hipStream_t st) {
    if (K < 1 || K > 64 || dom.m < 1 || dom.n < 2 || K > dom.n - 1 || dom.m > dom.n || Lp != (int64_t)dom.m * dom.n || !dom.rows || !dom.is_query) {
        pc_set_error("pc_launch_nn_select_rows: %d rows of %d genomes with %lld values, K = %d", dom.m, dom.n, (long long)Lp, K);
        return PC_ERR_ARG;
    }
    const nn_key flip = as_distance ? 0ull : ~0ull;
    hipLaunchKernelGGL(k_nn_qrows, dim3((unsigned)((dom.m + NN_WAVES - 1) / NN_WAVES)), dim3(NN_THREADS), 0, st, vals, dom, flip, K, key, nbr);
    int rc = nn_check("k_nn_qrows");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_nn_qcols, dim3((unsigned)((dom.n + NN_TILE - 1) / NN_TILE)), dim3(NN_THREADS), 0, st, vals, dom, flip, K, key, nbr);
    return nn_check("k_nn_qcols");
}
// The seed of pc_fill_rows_nearest, checked and packed on the host: seed_nbr / seed_val [N][k_seed], of which the first ks columns of
// every row g with !is_query[g] go into key / idx [N][K] (ks <= K); everything else is the sentinel.  The transform is nn_key_of's, in
// plain integer arithmetic.  Returns 0, or 1 (an entry that is out of range, a query genome or g itself) / 2 (a row that does not
// ascend in (key, index)) with the entry in *bad_g, *bad_j; nothing on the device is touched.
int pc_nn_seed_pack(const int32_t* seed_nbr, const double* seed_val, int k_seed, int ks, int N, int K, const uint8_t* is_query, int as_distance,
                    unsigned long long* key, int32_t* idx, int* bad_g, int* bad_j) {
    const nn_key flip = as_distance ? 0ull : ~0ull;
    for (int g = 0; g < N; ++g) {
        nn_key* const kr = key + (size_t)g * K; int32_t* const ir = idx + (size_t)g * K;
        for (int j = 0; j < K; ++j) { kr[j] = NN_WORST_KEY; ir[j] = NN_WORST_IDX; }
        if (is_query[g]) continue;
        for (int j = 0; j < ks; ++j) {
            const int32_t h = seed_nbr[(size_t)g * k_seed + j];
            nn_key u = 0;
            __builtin_memcpy(&u, &seed_val[(size_t)g * k_seed + j], 8);
            const nn_key kj = (u ^ ((u >> 63) ? ~0ull : (1ull << 63))) ^ flip;
            *bad_g = g; *bad_j = j;
            if (h < 0 || h >= N || h == g || is_query[h]) return 1;
            if (j > 0 && !(kr[j - 1] < kj || (kr[j - 1] == kj && ir[j - 1] < h))) return 2;
            kr[j] = kj; ir[j] = h;
        }
    }
    return 0;
}
// the column pass's tile edge (pc_nearest_rows_tile)
int pc_nn_rows_tile(void) { return NN_TILE; }

int pc_launch_nn_finish(const unsigned long long* key, double* val, int64_t n, int as_distance, hipStream_t st) {
    if (n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_nn_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, key, val, n, as_distance ? 0ull : ~0ull);
    return nn_check("k_nn_finish");
}

// dkey / dpos: [2 L]
int pc_launch_nn_pair_entries(const int32_t* src, const int32_t* tgt, unsigned long long* dkey, uint32_t* dpos, int64_t L, hipStream_t st) {
    if (L <= 0) return PC_OK;
    hipLaunchKernelGGL(k_nn_pair_entries, dim3((unsigned)((2 * L + 255) / 256)), dim3(256), 0, st, src, tgt, dkey, dpos, L);
    return nn_check("k_nn_pair_entries");
}
// skey / spos: the 2 L sorted entries; val: [L]; start: [N + 1]; key / nbr: [N][K], count: [N], 1 <= K <= 64, N >= 1
int pc_launch_nn_of_pairs(const unsigned long long* skey, const uint32_t* spos, const double* val, int64_t L, int N, int as_distance, int K,
                          uint32_t* start, unsigned long long* key, int32_t* nbr, int32_t* count, hipStream_t st) {
    if (K < 1 || K > 64 || N < 1 || L < 0 || L > ((int64_t)1 << 30)) {
        pc_set_error("pc_launch_nn_of_pairs: %lld pairs of %d genomes, K = %d", (long long)L, N, K);
        return PC_ERR_ARG;
    }
    hipLaunchKernelGGL(k_nn_run_starts, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, skey, 2 * L, N, start);
    int rc = nn_check("k_nn_run_starts");
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_nn_pairs, dim3((unsigned)((N + NN_WAVES - 1) / NN_WAVES)), dim3(NN_THREADS), 0, st, skey, spos, val, start, N,
                       as_distance ? 0ull : ~0ull, K, key, nbr, count);
    return nn_check("k_nn_pairs");
}

// key / nbr: [N][K]; fkey / fnbr: [n_foreign][N][K], 1 <= K <= 64
int pc_launch_nn_merge(unsigned long long* key, int32_t* nbr, const unsigned long long* fkey, const int32_t* fnbr, int n_foreign, int N, int K, hipStream_t st) {
    if (n_foreign <= 0 || N <= 0) return PC_OK;
    if (K < 1 || K > 64) { pc_set_error("pc_launch_nn_merge: K = %d", K); return PC_ERR_ARG; }
    hipLaunchKernelGGL(k_nn_merge, dim3((unsigned)((N + NN_WAVES - 1) / NN_WAVES)), dim3(NN_THREADS), 0, st, key, nbr, fkey, fnbr, n_foreign, N, K);
    return nn_check("k_nn_merge");
}
