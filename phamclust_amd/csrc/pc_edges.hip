// pc_edges.hip -- the edge-list kernels of pc_fill_edges and pc_fill_rows_edges: an order-preserving, two-pass stream compaction of a
// filled slab.  Two pass bodies, each written once over the slab's pair domain (pc_slab_pass.h: the chunks, the load, PcTriDomain for
// the triangular slab a fill writes with condensed = 0, PcRowsDomain for a rows slab):
//   pc_edge_count_body   elements of the chunk that are pairs of the call and pass the predicate (d <= thr for a distance fill,
//                        sim >= thr for a similarity fill: a plain f64 compare on the delivered, already round(x, 6) value) -> counts[chunk]
//   (pc_scan_exclusive_u32 over the counts: where each chunk's edges start, and the slab's total)
//   pc_edge_emit_body    re-reads the chunk and writes (s, t, value) of every such element at offs[chunk] + its rank in the chunk
// The kernels -- k_edge_count / k_edge_emit over a triangular slab, k_edge_count_rows / k_edge_emit_rows over a rows slab -- build the
// domain from their argument and call the body.  k_edge_count_bars / k_edge_emit_bars (pc_fill_edges_bars: a bar per genome in the
// threshold's place, triangular slabs only) are the same two passes written beside them; their section says what differs.
// Ranks come from wave ballots and a per-wave prefix in LDS, never from atomics: the output keeps element order.  On a triangular slab
// that is sorted by target, then source -- the order is part of pc_fill_edges' contract; on a rows slab it is row-major, by query row,
// then by the other genome, and the host sorts the call's edges by (target, source) once.  The reference's counterpart is the filter
// inside matrix_to_adjacency (matrix.py:536-551, skip_zero) and SymMatrix.nearest_neighbors (matrix.py:265-296), both over the
// dense matrix on the host.
// Both passes stream the slab from HBM once (emit skips chunks without an edge) and do nothing else that costs: the HBM rate is their
// only roofline (profiles/edges_fill.txt).
#include "pc_slab_pass.h"

int64_t pc_edge_chunks(int64_t Lp) { return (Lp + SLAB_CHUNK - 1) / SLAB_CHUNK; }
int pc_rows_slab_span(int pass) { return pass >= 0 && pass <= 2 ? SLAB_CHUNK : 0; }

template <int DIST> __device__ __forceinline__ bool pc_edge_pass(double v, double thr) { return DIST ? v <= thr : v >= thr; }

// (count names no pair: a domain that does not filter is never located)
template <int DIST, class Dom>
__device__ __forceinline__ void pc_edge_count_body(const double* __restrict__ vals, int64_t Lp, double thr, const Dom dom, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[SLAB_THREADS / 64];
    __shared__ typename Dom::Origin origin;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SLAB_CHUNK + (int64_t)threadIdx.x * 2;
    typename Dom::Cursor at{};
    if constexpr (Dom::kLocateFirst) {
        pc_slab_locate(dom, origin);
        __syncthreads();
        at = dom.start(origin);
    }
    uint32_t n = 0;                                    // the wave's count (the same in every lane)
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        double a, b;
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, a, b);
        const bool pa = have > 0 && pc_edge_pass<DIST>(a, thr) && dom.live(at, i);
        const bool pb = have > 1 && pc_edge_pass<DIST>(b, thr) && dom.live(at, i + 1);
        n += (uint32_t)__popcll(__ballot(pa)) + (uint32_t)__popcll(__ballot(pb));
        dom.step(at);
    }
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < SLAB_THREADS / 64; ++w) tot += wsum[w];
        counts[blockIdx.x] = tot;
    }
}

template <int DIST, class Dom>
__device__ __forceinline__ void pc_edge_emit_body(const double* __restrict__ vals, int64_t Lp, double thr, const Dom dom, const uint32_t* __restrict__ offs,
                                                  int32_t* __restrict__ src, int32_t* __restrict__ tgt, double* __restrict__ val) {
    __shared__ uint32_t wcnt[SLAB_ITERS][SLAB_THREADS / 64];
    __shared__ typename Dom::Origin origin;
    const uint32_t off = offs[blockIdx.x];
    if (offs[blockIdx.x + 1] == off) return;           // (the whole workgroup: no edge in this chunk, nothing to re-read)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SLAB_CHUNK + (int64_t)threadIdx.x * 2;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    typename Dom::Cursor at{};
    if constexpr (Dom::kLocateFirst) {
        pc_slab_locate(dom, origin);
        __syncthreads();
        at = dom.start(origin);
    }
    const typename Dom::Cursor first = at;
    double va[SLAB_ITERS], vb[SLAB_ITERS];
    uint32_t pre[SLAB_ITERS];                          // passing elements of the wave's iteration j before this thread's first one, in ELEMENT order
    uint32_t pass_a = 0, pass_b = 0;
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, va[j], vb[j]);
        const bool pa = have > 0 && pc_edge_pass<DIST>(va[j], thr) && dom.live(at, i);
        const bool pb = have > 1 && pc_edge_pass<DIST>(vb[j], thr) && dom.live(at, i + 1);
        const unsigned long long ba = __ballot(pa), bb = __ballot(pb);
        // lane l holds elements 2 l and 2 l + 1 of the wave's 128: both slots of every lower lane come before this thread's first
        pre[j] = (uint32_t)__popcll(ba & below) + (uint32_t)__popcll(bb & below);
        pass_a |= (uint32_t)pa << j; pass_b |= (uint32_t)pb << j;
        if (lane == 0) wcnt[j][wv] = (uint32_t)__popcll(ba) + (uint32_t)__popcll(bb);
        dom.step(at);
    }
    if constexpr (!Dom::kLocateFirst) pc_slab_locate(dom, origin);
    __syncthreads();
    if constexpr (Dom::kLocateFirst) at = first; else at = dom.start(origin);
    uint32_t run = off;
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        uint32_t o = run;
#pragma unroll
        for (int w = 0; w < SLAB_THREADS / 64; ++w) { const uint32_t c = wcnt[j][w]; if (w < wv) o += c; run += c; }
        o += pre[j];
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        int a, b, s, t;
        if ((pass_a >> j) & 1u) {
            dom.pair(at, i, a, b); Dom::sorted(a, b, s, t);
            src[o] = s; tgt[o] = t; val[o] = va[j];
            ++o;
        }
        if ((pass_b >> j) & 1u) {
            dom.pair(at, i + 1, a, b); Dom::sorted(a, b, s, t);
            src[o] = s; tgt[o] = t; val[o] = vb[j];
        }
        dom.step(at);
    }
}

template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_edge_count(const double* __restrict__ vals, int64_t Lp, double thr, uint32_t* __restrict__ counts) {
    pc_edge_count_body<DIST>(vals, Lp, thr, PcTriDomain{}, counts);
}
template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_edge_emit(const double* __restrict__ vals, int64_t Lp, double thr, PcShard sh,
                                                            const uint32_t* __restrict__ offs, int32_t* __restrict__ src,
                                                            int32_t* __restrict__ tgt, double* __restrict__ val) {
    pc_edge_emit_body<DIST>(vals, Lp, thr, PcTriDomain{sh}, offs, src, tgt, val);
}
template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_edge_count_rows(const double* __restrict__ vals, int64_t Lp, double thr, PcRowsSlab dom,
                                                                  uint32_t* __restrict__ counts) {
    pc_edge_count_body<DIST>(vals, Lp, thr, PcRowsDomain{dom}, counts);
}
template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_edge_emit_rows(const double* __restrict__ vals, int64_t Lp, double thr, PcRowsSlab dom,
                                                                 const uint32_t* __restrict__ offs, int32_t* __restrict__ src,
                                                                 int32_t* __restrict__ tgt, double* __restrict__ val) {
    pc_edge_emit_body<DIST>(vals, Lp, thr, PcRowsDomain{dom}, offs, src, tgt, val);
}

// ---- pc_fill_edges_bars: the same two passes with a bar per genome instead of one threshold.  Element (s, t) passes when its value
// passes bar[s] OR bar[t], so BOTH passes name their pairs: the chunk is located ahead of the loads (one binary search per workgroup,
// one barrier), and the forward walk of PcTriDomain::pair gives (s, t) per element.  Along a slab row t is fixed and s runs
// consecutively: bar[t] is one address for long runs of a wave's lanes, bar[s] an 8-byte load per element that coalesces as the
// value's own does.  bar[N] stays resident for the call; nothing of it is read beyond the genomes of an element that exists.
// Triangular slabs only (the rows forms take one threshold).  Ranks as above: ballots and a per-wave prefix in LDS, no atomics.
template <int DIST> __device__ __forceinline__ bool pc_edge_pass_bars(double v, const double* __restrict__ bar, int s, int t) {
    return pc_edge_pass<DIST>(v, bar[s]) || pc_edge_pass<DIST>(v, bar[t]);
}

template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_edge_count_bars(const double* __restrict__ vals, int64_t Lp, const double* __restrict__ bar, PcShard sh,
                                                                  uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[SLAB_THREADS / 64];
    __shared__ PcTriDomain::Origin origin;
    const PcTriDomain dom{sh};
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SLAB_CHUNK + (int64_t)threadIdx.x * 2;
    pc_slab_locate(dom, origin);
    __syncthreads();
    PcTriDomain::Cursor at = dom.start(origin);
    uint32_t n = 0;                                    // the wave's count (the same in every lane)
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        double a, b;
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, a, b);
        bool pa = false, pb = false;
        int s, t;
        if (have > 0) { dom.pair(at, i, t, s); pa = pc_edge_pass_bars<DIST>(a, bar, s, t); }
        if (have > 1) { dom.pair(at, i + 1, t, s); pb = pc_edge_pass_bars<DIST>(b, bar, s, t); }
        n += (uint32_t)__popcll(__ballot(pa)) + (uint32_t)__popcll(__ballot(pb));
        dom.step(at);
    }
    if (lane == 0) wsum[wv] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < SLAB_THREADS / 64; ++w) tot += wsum[w];
        counts[blockIdx.x] = tot;
    }
}

template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_edge_emit_bars(const double* __restrict__ vals, int64_t Lp, const double* __restrict__ bar, PcShard sh,
                                                                 const uint32_t* __restrict__ offs, int32_t* __restrict__ src, int32_t* __restrict__ tgt,
                                                                 double* __restrict__ val) {
    __shared__ uint32_t wcnt[SLAB_ITERS][SLAB_THREADS / 64];
    __shared__ PcTriDomain::Origin origin;
    const PcTriDomain dom{sh};
    const uint32_t off = offs[blockIdx.x];
    if (offs[blockIdx.x + 1] == off) return;           // (the whole workgroup: no edge in this chunk, nothing to re-read)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SLAB_CHUNK + (int64_t)threadIdx.x * 2;
    const unsigned long long below = ((unsigned long long)1 << lane) - 1;
    pc_slab_locate(dom, origin);
    __syncthreads();
    PcTriDomain::Cursor at = dom.start(origin);
    const PcTriDomain::Cursor first = at;
    double va[SLAB_ITERS], vb[SLAB_ITERS];
    uint32_t pre[SLAB_ITERS];                          // passing elements of the wave's iteration j before this thread's first one, in ELEMENT order
    uint32_t pass_a = 0, pass_b = 0;
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, va[j], vb[j]);
        bool pa = false, pb = false;
        int s, t;
        if (have > 0) { dom.pair(at, i, t, s); pa = pc_edge_pass_bars<DIST>(va[j], bar, s, t); }
        if (have > 1) { dom.pair(at, i + 1, t, s); pb = pc_edge_pass_bars<DIST>(vb[j], bar, s, t); }
        const unsigned long long ba = __ballot(pa), bb = __ballot(pb);
        pre[j] = (uint32_t)__popcll(ba & below) + (uint32_t)__popcll(bb & below);
        pass_a |= (uint32_t)pa << j; pass_b |= (uint32_t)pb << j;
        if (lane == 0) wcnt[j][wv] = (uint32_t)__popcll(ba) + (uint32_t)__popcll(bb);
        dom.step(at);
    }
    __syncthreads();
    at = first;                                        // (elements are asked in ascending order again)
    uint32_t run = off;
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        uint32_t o = run;
#pragma unroll
        for (int w = 0; w < SLAB_THREADS / 64; ++w) { const uint32_t c = wcnt[j][w]; if (w < wv) o += c; run += c; }
        o += pre[j];
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        int s, t;
        if ((pass_a >> j) & 1u) {
            dom.pair(at, i, t, s);
            src[o] = s; tgt[o] = t; val[o] = va[j];
            ++o;
        }
        if ((pass_b >> j) & 1u) {
            dom.pair(at, i + 1, t, s);
            src[o] = s; tgt[o] = t; val[o] = vb[j];
        }
        dom.step(at);
    }
}

// counts: [pc_edge_chunks(Lp)] (the caller keeps one more element, zero, for the scan's total); dom: the slab's shard or rows domain,
// its tables on the device
int pc_launch_edge_count(const double* vals, int64_t Lp, int as_distance, double thr, PcSlabDomain dom, uint32_t* counts, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const char* const what = dom.is_rows ? "k_edge_count_rows" : "k_edge_count";
    const int rc = pc_slab_domain_check(dom, Lp, what);
    if (rc != PC_OK) return rc;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1>(as_distance ? 1 : 0, [&](auto dist) {
        constexpr int DIST = decltype(dist)::value;
        if (dom.is_rows) hipLaunchKernelGGL(k_edge_count_rows<DIST>, grid, block, 0, st, vals, Lp, thr, dom.rows, counts);
        else hipLaunchKernelGGL(k_edge_count<DIST>, grid, block, 0, st, vals, Lp, thr, counts);
    });
    return pc_launch_check(what);
}
// offs: [pc_edge_chunks(Lp) + 1], the exclusive scan of the counts
int pc_launch_edge_emit(const double* vals, int64_t Lp, int as_distance, double thr, PcSlabDomain dom, const uint32_t* offs,
                        int32_t* src, int32_t* tgt, double* val, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const char* const what = dom.is_rows ? "k_edge_emit_rows" : "k_edge_emit";
    const int rc = pc_slab_domain_check(dom, Lp, what);
    if (rc != PC_OK) return rc;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1>(as_distance ? 1 : 0, [&](auto dist) {
        constexpr int DIST = decltype(dist)::value;
        if (dom.is_rows) hipLaunchKernelGGL(k_edge_emit_rows<DIST>, grid, block, 0, st, vals, Lp, thr, dom.rows, offs, src, tgt, val);
        else hipLaunchKernelGGL(k_edge_emit<DIST>, grid, block, 0, st, vals, Lp, thr, dom.shard, offs, src, tgt, val);
    });
    return pc_launch_check(what);
}
// the same two launches with a bar per genome: bar f64[N] on the device, N above every genome of the shard; a triangular slab only
int pc_launch_edge_count_bars(const double* vals, int64_t Lp, int as_distance, const double* bar, const PcShard& sh, uint32_t* counts, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1>(as_distance ? 1 : 0, [&](auto dist) {
        hipLaunchKernelGGL(k_edge_count_bars<decltype(dist)::value>, grid, block, 0, st, vals, Lp, bar, sh, counts);
    });
    return pc_launch_check("k_edge_count_bars");
}
int pc_launch_edge_emit_bars(const double* vals, int64_t Lp, int as_distance, const double* bar, const PcShard& sh, const uint32_t* offs,
                             int32_t* src, int32_t* tgt, double* val, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1>(as_distance ? 1 : 0, [&](auto dist) {
        hipLaunchKernelGGL(k_edge_emit_bars<decltype(dist)::value>, grid, block, 0, st, vals, Lp, bar, sh, offs, src, tgt, val);
    });
    return pc_launch_check("k_edge_emit_bars");
}
