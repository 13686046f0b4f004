// pc_edges.hip -- the edge-list kernels of pc_fill_edges: an order-preserving, two-pass stream compaction of a filled slab.
// The slab is what a fill writes with condensed = 0 (shard layout: the values of pairs (s, owned[k]), s = 0 .. owned[k] - 1, at
// lbase[k] + s); both kernels see it as one flat f64[Lp] cut into chunks of EDGE_CHUNK elements, one workgroup each:
//   k_edge_count   elements of the chunk that pass the predicate (d <= thr for a distance fill, sim >= thr for a similarity fill:
//                  a plain f64 compare on the delivered, already round(x, 6) value) -> counts[chunk]
//   (pc_scan_exclusive_u32 over the counts: where each chunk's edges start, and the slab's total)
//   k_edge_emit    re-reads the chunk and writes (s, t, value) of every passing element at offs[chunk] + its rank in the chunk
// Ranks come from wave ballots and a per-wave prefix in LDS, never from atomics: the output keeps element order, i.e. it is
// sorted by target, then source -- the order is part of pc_fill_edges' contract.  The reference's counterpart is the filter
// inside matrix_to_adjacency (matrix.py:536-551, skip_zero) and SymMatrix.nearest_neighbors (matrix.py:265-296), both over the
// dense matrix on the host.
// Both kernels stream the slab from HBM once (k_edge_emit skips chunks without an edge) and do nothing else that costs: the HBM
// rate is their only roofline (profiles/edges_fill.txt).
#include "pc_pairs.h"

#define EDGE_THREADS 256
#define EDGE_ITERS 8
#define EDGE_STRIDE (EDGE_THREADS * 2)                 // elements the workgroup reads per iteration: two consecutive ones per thread (one 16-byte load)
#define EDGE_CHUNK (EDGE_STRIDE * EDGE_ITERS)          // 4,096 elements = 32 KB of slab per workgroup

int64_t pc_edge_chunks(int64_t Lp) { return (Lp + EDGE_CHUNK - 1) / EDGE_CHUNK; }

template <int DIST> __device__ __forceinline__ bool pc_edge_pass(double v, double thr) { return DIST ? v <= thr : v >= thr; }

// elements i and i + 1 of the slab (i even: the slab's base is an allocation's, chunks and thread slots are even, so the 16-byte
// load is aligned); the last element of an odd Lp is loaded alone, nothing is read beyond Lp.  Returns how many of the two exist.
__device__ __forceinline__ int pc_edge_load(const double* __restrict__ vals, int64_t i, int64_t Lp, double& a, double& b) {
    a = b = 0.0;
    if (i + 1 < Lp) {
        const double2 v = *reinterpret_cast<const double2*>(vals + i);
        a = v.x; b = v.y;
        return 2;
    }
    if (i < Lp) { a = vals[i]; return 1; }
    return 0;
}

template <int DIST>
__global__ __launch_bounds__(EDGE_THREADS) void k_edge_count(const double* __restrict__ vals, int64_t Lp, double thr, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[EDGE_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * EDGE_CHUNK + (int64_t)threadIdx.x * 2;
    uint32_t n = 0;                                    // the wave's count (the same in every lane)
#pragma unroll
    for (int j = 0; j < EDGE_ITERS; ++j) {
        double a, b;
        const int have = pc_edge_load(vals, base + (int64_t)j * EDGE_STRIDE, Lp, a, b);
        const bool pa = have > 0 && pc_edge_pass<DIST>(a, thr), pb = have > 1 && pc_edge_pass<DIST>(b, thr);
        n += (uint32_t)__popcll(__ballot(pa)) + (uint32_t)__popcll(__ballot(pb));
    }
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < EDGE_THREADS / 64; ++w) tot += wsum[w];
        counts[blockIdx.x] = tot;
    }
}

template <int DIST>
__global__ __launch_bounds__(EDGE_THREADS) void k_edge_emit(const double* __restrict__ vals, int64_t Lp, double thr, PcShard sh,
                                                            const uint32_t* __restrict__ offs, int32_t* __restrict__ src,
                                                            int32_t* __restrict__ tgt, double* __restrict__ val) {
    __shared__ uint32_t wcnt[EDGE_ITERS][EDGE_THREADS / 64];
    __shared__ int k_first;
    const uint32_t off = offs[blockIdx.x];
    if (offs[blockIdx.x + 1] == off) return;           // (the whole workgroup: no edge in this chunk, nothing to re-read)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * EDGE_CHUNK, base = i0 + (int64_t)threadIdx.x * 2;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    double va[EDGE_ITERS], vb[EDGE_ITERS];
    uint32_t pre[EDGE_ITERS];                          // passing elements of the wave's iteration j before this thread's first one, in ELEMENT order
    uint32_t pass_a = 0, pass_b = 0;
#pragma unroll
    for (int j = 0; j < EDGE_ITERS; ++j) {
        const int have = pc_edge_load(vals, base + (int64_t)j * EDGE_STRIDE, Lp, va[j], vb[j]);
        const bool pa = have > 0 && pc_edge_pass<DIST>(va[j], thr), pb = have > 1 && pc_edge_pass<DIST>(vb[j], thr);
        const unsigned long long ba = __ballot(pa), bb = __ballot(pb);
        // lane l holds elements 2 l and 2 l + 1 of the wave's 128: both slots of every lower lane come before this thread's first
        pre[j] = (uint32_t)__popcll(ba & below) + (uint32_t)__popcll(bb & below);
        pass_a |= (uint32_t)pa << j; pass_b |= (uint32_t)pb << j;
        if (lane == 0) wcnt[j][wv] = (uint32_t)__popcll(ba) + (uint32_t)__popcll(bb);
    }
    if (threadIdx.x == 0) {
        // the row of the chunk's first element: lbase[k] <= i0 < lbase[k + 1] (lbase[0] = 0 <= i0 < Lp = lbase[nown]); rows of
        // length 0 repeat an lbase value and can never be the answer
        int lo = 0, hi = sh.nown;
        while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (sh.lbase[mid] <= i0) lo = mid; else hi = mid; }
        k_first = lo;
    }
    __syncthreads();
    int k = k_first;
    uint32_t run = off;
#pragma unroll
    for (int j = 0; j < EDGE_ITERS; ++j) {
        uint32_t at = run;
#pragma unroll
        for (int w = 0; w < EDGE_THREADS / 64; ++w) { const uint32_t c = wcnt[j][w]; if (w < wv) at += c; run += c; }
        at += pre[j];
        const int64_t i = base + (int64_t)j * EDGE_STRIDE;
        if ((pass_a >> j) & 1u) {                      // (a passing element lies below Lp = lbase[nown]: the walk stops at k + 1 <= nown)
            while (i >= sh.lbase[k + 1]) ++k;
            src[at] = (int32_t)(i - sh.lbase[k]); tgt[at] = sh.owned[k]; val[at] = va[j];
            ++at;
        }
        if ((pass_b >> j) & 1u) {
            while (i + 1 >= sh.lbase[k + 1]) ++k;
            src[at] = (int32_t)(i + 1 - sh.lbase[k]); tgt[at] = sh.owned[k]; val[at] = vb[j];
        }
    }
}

// ---- the same two passes over a rows slab (PcRowsSlab: vals = f64[m][n] seen flat, Lp = m * n; pc_fill_rows_edges): an element counts
// iff it is LIVE (pc_rows_live) and passes.  The same chunks, loads and ballot ranking; where the triangular kernels find (s, t) by
// lbase, these carry (row, column) in a PcRowsCursor.  Output order is element order: row-major, so by query row, then by the other
// genome -- the host sorts the call's edges by (target, source) once.
template <int DIST>
__global__ __launch_bounds__(EDGE_THREADS) void k_edge_count_rows(const double* __restrict__ vals, int64_t Lp, double thr, PcRowsSlab dom,
                                                                  uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[EDGE_THREADS / 64];
    __shared__ int2 origin;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * EDGE_CHUNK, base = i0 + (int64_t)threadIdx.x * 2;
    if (threadIdx.x == 0) origin = pc_rows_origin(i0, dom.n);
    __syncthreads();
    PcRowsCursor at;
    at.start(origin, threadIdx.x * 2u, dom);
    uint32_t n = 0;                                    // the wave's count (the same in every lane)
#pragma unroll
    for (int j = 0; j < EDGE_ITERS; ++j) {
        double a, b;
        const int have = pc_edge_load(vals, base + (int64_t)j * EDGE_STRIDE, Lp, a, b);
        int row1, col1, q;
        at.next(dom, row1, col1);
        const bool pa = have > 0 && pc_edge_pass<DIST>(a, thr) && pc_rows_live(dom, at.row, at.col, q);
        const bool pb = have > 1 && pc_edge_pass<DIST>(b, thr) && pc_rows_live(dom, row1, col1, q);
        n += (uint32_t)__popcll(__ballot(pa)) + (uint32_t)__popcll(__ballot(pb));
        at.advance(dom);
    }
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < EDGE_THREADS / 64; ++w) tot += wsum[w];
        counts[blockIdx.x] = tot;
    }
}

template <int DIST>
__global__ __launch_bounds__(EDGE_THREADS) void k_edge_emit_rows(const double* __restrict__ vals, int64_t Lp, double thr, PcRowsSlab dom,
                                                                 const uint32_t* __restrict__ offs, int32_t* __restrict__ src,
                                                                 int32_t* __restrict__ tgt, double* __restrict__ val) {
    __shared__ uint32_t wcnt[EDGE_ITERS][EDGE_THREADS / 64];
    __shared__ int2 origin;
    const uint32_t off = offs[blockIdx.x];
    if (offs[blockIdx.x + 1] == off) return;           // (the whole workgroup: no edge in this chunk, nothing to re-read)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * EDGE_CHUNK, base = i0 + (int64_t)threadIdx.x * 2;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    if (threadIdx.x == 0) origin = pc_rows_origin(i0, dom.n);
    __syncthreads();
    PcRowsCursor first, at;
    first.start(origin, threadIdx.x * 2u, dom);
    at = first;
    double va[EDGE_ITERS], vb[EDGE_ITERS];
    uint32_t pre[EDGE_ITERS];                          // passing elements of the wave's iteration j before this thread's first one, in ELEMENT order
    uint32_t pass_a = 0, pass_b = 0;
#pragma unroll
    for (int j = 0; j < EDGE_ITERS; ++j) {
        const int have = pc_edge_load(vals, base + (int64_t)j * EDGE_STRIDE, Lp, va[j], vb[j]);
        int row1, col1, q;
        at.next(dom, row1, col1);
        const bool pa = have > 0 && pc_edge_pass<DIST>(va[j], thr) && pc_rows_live(dom, at.row, at.col, q);
        const bool pb = have > 1 && pc_edge_pass<DIST>(vb[j], thr) && pc_rows_live(dom, row1, col1, q);
        const unsigned long long ba = __ballot(pa), bb = __ballot(pb);
        pre[j] = (uint32_t)__popcll(ba & below) + (uint32_t)__popcll(bb & below);
        pass_a |= (uint32_t)pa << j; pass_b |= (uint32_t)pb << j;
        if (lane == 0) wcnt[j][wv] = (uint32_t)__popcll(ba) + (uint32_t)__popcll(bb);
        at.advance(dom);
    }
    __syncthreads();
    at = first;
    uint32_t run = off;
#pragma unroll
    for (int j = 0; j < EDGE_ITERS; ++j) {
        uint32_t o = run;
#pragma unroll
        for (int w = 0; w < EDGE_THREADS / 64; ++w) { const uint32_t c = wcnt[j][w]; if (w < wv) o += c; run += c; }
        o += pre[j];
        if ((pass_a >> j) & 1u) {                      // (a passing element lies below Lp = m * n: its row is one of the slab's)
            const int q = dom.rows[at.row], g = at.col;
            src[o] = q < g ? q : g; tgt[o] = q < g ? g : q; val[o] = va[j];
            ++o;
        }
        if ((pass_b >> j) & 1u) {
            int row1, col1;
            at.next(dom, row1, col1);
            const int q = dom.rows[row1], g = col1;
            src[o] = q < g ? q : g; tgt[o] = q < g ? g : q; val[o] = vb[j];
        }
        at.advance(dom);
    }
}

// elements one workgroup of a rows pass covers: the three units' chunks are the same 4,096 (each asserts it)
static_assert(EDGE_CHUNK == 4096, "pc_rows_slab_span");
int pc_rows_slab_span(int pass) { return pass >= 0 && pass <= 2 ? EDGE_CHUNK : 0; }

static int edge_rows_dom(PcRowsSlab& dom, int64_t Lp, const char* what) {
    if (dom.n <= 0 || dom.m <= 0 || Lp != (int64_t)dom.m * dom.n) { pc_set_error("%s: a rows slab of %d x %d is not %lld values", what, dom.m, dom.n, (long long)Lp); return PC_ERR_ARG; }
    dom.adv_rows = EDGE_STRIDE / dom.n; dom.adv_cols = EDGE_STRIDE % dom.n;
    return PC_OK;
}
// counts: [pc_edge_chunks(Lp)] as for pc_launch_edge_count; dom: rows / is_query on the device, Lp = m * n
int pc_launch_edge_count_rows(const double* vals, int64_t Lp, int as_distance, double thr, PcRowsSlab dom, uint32_t* counts, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    int rc = edge_rows_dom(dom, Lp, "k_edge_count_rows");
    if (rc != PC_OK) return rc;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(EDGE_THREADS);
    if (as_distance) hipLaunchKernelGGL(k_edge_count_rows<1>, grid, block, 0, st, vals, Lp, thr, dom, counts);
    else hipLaunchKernelGGL(k_edge_count_rows<0>, grid, block, 0, st, vals, Lp, thr, dom, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_edge_count_rows launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
int pc_launch_edge_emit_rows(const double* vals, int64_t Lp, int as_distance, double thr, PcRowsSlab dom, const uint32_t* offs,
                             int32_t* src, int32_t* tgt, double* val, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    int rc = edge_rows_dom(dom, Lp, "k_edge_emit_rows");
    if (rc != PC_OK) return rc;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(EDGE_THREADS);
    if (as_distance) hipLaunchKernelGGL(k_edge_emit_rows<1>, grid, block, 0, st, vals, Lp, thr, dom, offs, src, tgt, val);
    else hipLaunchKernelGGL(k_edge_emit_rows<0>, grid, block, 0, st, vals, Lp, thr, dom, offs, src, tgt, val);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_edge_emit_rows launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// counts: [pc_edge_chunks(Lp)] (the caller keeps one more element, zero, for the scan's total)
int pc_launch_edge_count(const double* vals, int64_t Lp, int as_distance, double thr, uint32_t* counts, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(EDGE_THREADS);
    if (as_distance) hipLaunchKernelGGL(k_edge_count<1>, grid, block, 0, st, vals, Lp, thr, counts);
    else hipLaunchKernelGGL(k_edge_count<0>, grid, block, 0, st, vals, Lp, thr, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_edge_count launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
// offs: [pc_edge_chunks(Lp) + 1], the exclusive scan of the counts; sh: the slab's shard (owned / lbase on the device, nown targets)
int pc_launch_edge_emit(const double* vals, int64_t Lp, int as_distance, double thr, const PcShard& sh, const uint32_t* offs,
                        int32_t* src, int32_t* tgt, double* val, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(EDGE_THREADS);
    if (as_distance) hipLaunchKernelGGL(k_edge_emit<1>, grid, block, 0, st, vals, Lp, thr, sh, offs, src, tgt, val);
    else hipLaunchKernelGGL(k_edge_emit<0>, grid, block, 0, st, vals, Lp, thr, sh, offs, src, tgt, val);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_edge_emit launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
