// pc_components.hip -- the kernels of pc_fill_components: the connected components of the graph whose edges are the pairs of a
// filled slab that pass a threshold, by a lock-free union-find over parent[N] (i32, device-resident across the call's slabs).
// With a strict distance predicate (d < eps) the components ARE the reference's single-linkage clusters at eps
// (clustering.py:4-51: AgglomerativeClustering(linkage="single", distance_threshold=eps) merges below eps, never at it), and every
// average / complete cluster at eps lies inside one of them.
//   k_cc_init     parent[g] = g, the pair counter = 0                                   (once per call)
//   k_cc_union    ONE body, pc_cc_union_body, under two kernels: k_cc_union over a triangular slab (PcTriDomain) and k_cc_union_rows
//                 over a rows slab (PcRowsDomain; pc_fill_rows_components, where parent[] may come in seeded with a stored labelling,
//                 parent[g] = the smallest member of g's stored component <= g: I1 and I2 hold for it as for the identity).  It
//                 streams the slab as every slab pass does (pc_slab_pass.h: flat f64[Lp], chunks of 4,096 elements, 256 threads, eight
//                 16-byte loads per thread, the odd last element alone, nothing read beyond Lp) and asks the domain which elements
//                 are pairs and which two genomes a passing one joins; per passing pair: find both roots, equal -> done, else hook the
//                 LARGER root under the SMALLER by compare-and-swap
//   k_cc_merge    several devices, each with the forest of its own stretch of targets (pc_multi_fill_components): thread g unites g
//                 with its parent in every foreign forest fparent[f][n].  By I1 that parent p <= g is a node of g's foreign component,
//                 and the edges (g, fparent[g]) span every foreign component, so the root's forest ends up with exactly the components
//                 of the union of all devices' passing pairs; pc_cc_unite hooks larger under smaller, so I1 / I2 go on holding.
//   k_cc_labels   pointer jumping, launched ceil(log2 N) times after the last slab: labels[g] = the root of g
// Two invariants carry the correctness argument:
//   I1  parent[x] <= x, always.  (init: equal; a hook writes lo < hi into parent[hi]; a shortening writes an ancestor, which by I1
//       is smaller still.)  So every walk towards a root strictly descends: it ends after at most x steps, and no cycle can form.
//   I2  a word only ever decreases (CAS hi -> lo < hi; atomicMin), so a non-root (parent[x] < x) never becomes a root again.
// From them: a value ever read from parent[x], however stale, is a node of x's component and <= x, so a walk over stale values
// still ends at a node of the component that WAS a root; whether it still is one is decided by the CAS alone, which succeeds
// only on a root (parent[hi] == hi) and joins two different trees (lo < hi keeps the forest acyclic).  A pair is done when both
// walks met in one node or its own CAS succeeded -- connected either way -- and connections are never undone (a shortening
// replaces a parent by an ancestor).  The smallest genome m of a component has parent[m] <= m inside the component, i.e. is its
// root: labels are the smallest member's index, whatever order the races resolved in.
// Memory: inside the union pass EVERY access to parent[] is a relaxed agent-scope atomic (__hip_atomic_load, atomicCAS, atomicMin;
// no plain load or store): the XCDs' L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's writes.
// Progress: no workgroup ever waits for another.  The only loops are the walk (bounded by I1) and the CAS retry, whose larger
// root strictly descends with every round (a failed CAS returns the word's true value, < hi, and the walks go on from there).
// No flags, no spinning on a value another wave is to write, no sleeping.
#include "pc_slab_pass.h"

template <int DIST, int STRICT> __device__ __forceinline__ bool pc_cc_pass(double v, double thr) {
    if (DIST) return STRICT ? v < thr : v <= thr;
    return STRICT ? v > thr : v >= thr;
}

__device__ __forceinline__ int pc_cc_read(int32_t* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above x, halving the path on the way: a node v whose parent p is not a root gets its grandparent (atomicMin on a
// non-root only -- p < v was read, so by I2 v is none; gp < p by I1: the word decreases)
__device__ __forceinline__ int pc_cc_find(int32_t* parent, int x) {
    int v = x, p = pc_cc_read(parent, v);
    while (p != v) {
        const int gp = pc_cc_read(parent, p);
        if (gp != p) atomicMin(parent + v, gp);
        v = p; p = gp;
    }
    return v;
}

__device__ __forceinline__ void pc_cc_unite(int32_t* parent, int x, int y) {
    int a = pc_cc_find(parent, x), b = pc_cc_find(parent, y);
    while (a != b) {                                   // (most pairs of a dense component never enter)
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) break;                          // hooked: hi was a root, and is none from now on
        a = pc_cc_find(parent, was);                   // somebody else hooked hi (or the walk read a stale root): was < hi is its parent
        b = pc_cc_find(parent, lo);                    // a, b < hi: the larger root descends with every round
    }
}

__global__ __launch_bounds__(256) void k_cc_init(int32_t* __restrict__ parent, int n, unsigned long long* __restrict__ n_pass) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < n) parent[g] = g;
    if (g == 0) *n_pass = 0ull;
}

// the passing pairs of the chunk counted (one 64-bit add per workgroup) and united
template <int DIST, int STRICT, class Dom>
__device__ __forceinline__ void pc_cc_union_body(const double* __restrict__ vals, int64_t Lp, double thr, const Dom dom, int32_t* parent,
                                                 unsigned long long* n_pass) {
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
    const typename Dom::Cursor first = at;
    uint32_t n = 0;                                    // the wave's count (the same in every lane)
    uint32_t pass_a = 0, pass_b = 0;
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        double a, b;
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, a, b);
        const bool pa = have > 0 && pc_cc_pass<DIST, STRICT>(a, thr) && dom.live(at, i);
        const bool pb = have > 1 && pc_cc_pass<DIST, STRICT>(b, thr) && dom.live(at, i + 1);
        n += (uint32_t)__popcll(__ballot(pa)) + (uint32_t)__popcll(__ballot(pb));
        pass_a |= (uint32_t)pa << j; pass_b |= (uint32_t)pb << j;
        dom.step(at);
    }
    if (lane == 0) wsum[wv] = n;
    if constexpr (!Dom::kLocateFirst) pc_slab_locate(dom, origin);
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < SLAB_THREADS / 64; ++w) tot += wsum[w];
    if (tot == 0) return;                              // (the whole workgroup)
    if (threadIdx.x == 0) atomicAdd(n_pass, (unsigned long long)tot);
    if ((pass_a | pass_b) == 0) return;
    if constexpr (Dom::kLocateFirst) at = first; else at = dom.start(origin);
#pragma unroll 1
    for (int j = 0; j < SLAB_ITERS; ++j) {
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        int a, b;                                      // (the union takes a pair's genomes in either order)
        if ((pass_a >> j) & 1u) { dom.pair(at, i, a, b); pc_cc_unite(parent, b, a); }
        if ((pass_b >> j) & 1u) { dom.pair(at, i + 1, a, b); pc_cc_unite(parent, b, a); }
        dom.step(at);
    }
}

template <int DIST, int STRICT>
__global__ __launch_bounds__(SLAB_THREADS) void k_cc_union(const double* __restrict__ vals, int64_t Lp, double thr, PcShard sh,
                                                           int32_t* parent, unsigned long long* n_pass) {
    pc_cc_union_body<DIST, STRICT>(vals, Lp, thr, PcTriDomain{sh}, parent, n_pass);
}
template <int DIST, int STRICT>
__global__ __launch_bounds__(SLAB_THREADS) void k_cc_union_rows(const double* __restrict__ vals, int64_t Lp, double thr, PcRowsSlab dom,
                                                                int32_t* parent, unsigned long long* n_pass) {
    pc_cc_union_body<DIST, STRICT>(vals, Lp, thr, PcRowsDomain{dom}, parent, n_pass);
}

// the same relaxed agent-scope atomics on parent[] as k_cc_union (through pc_cc_unite); the foreign forests are read-only here
__global__ __launch_bounds__(256) void k_cc_merge(int32_t* parent, const int32_t* __restrict__ fparent, int n_foreign, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    for (int f = 0; f < n_foreign; ++f) {
        const int p = fparent[(size_t)f * n + g];
        if (p != g) pc_cc_unite(parent, g, p);
    }
}

// one round of pointer jumping (a launch of its own: plain accesses).  Thread g alone writes parent[g]; the grandparent it reads is
// the old one or one already jumped, an ancestor either way, so a node of depth d is at depth <= ceil(d / 2) afterwards.
__global__ __launch_bounds__(256) void k_cc_labels(int32_t* parent, int32_t* __restrict__ labels, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int r = parent[parent[g]];
    parent[g] = r;
    labels[g] = r;
}

int pc_launch_cc_init(int32_t* parent, int n, unsigned long long* n_pass, hipStream_t st) {
    hipLaunchKernelGGL(k_cc_init, dim3((unsigned)((std::max(n, 1) + 255) / 256)), dim3(256), 0, st, parent, n, n_pass);
    return pc_launch_check("k_cc_init");
}

// dom: the slab's shard or rows domain, its tables on the device; parent: [N], N above every genome of the slab's pairs
int pc_launch_cc_union(const double* vals, int64_t Lp, int as_distance, int strict, double thr, PcSlabDomain dom, int32_t* parent,
                       unsigned long long* n_pass, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const char* const what = dom.is_rows ? "k_cc_union_rows" : "k_cc_union";
    const int rc = pc_slab_domain_check(dom, Lp, what);
    if (rc != PC_OK) return rc;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1, 2, 3>((as_distance ? 2 : 0) + (strict ? 1 : 0), [&](auto form) {
        constexpr int DIST = decltype(form)::value >> 1, STRICT = decltype(form)::value & 1;
        if (dom.is_rows) hipLaunchKernelGGL((k_cc_union_rows<DIST, STRICT>), grid, block, 0, st, vals, Lp, thr, dom.rows, parent, n_pass);
        else hipLaunchKernelGGL((k_cc_union<DIST, STRICT>), grid, block, 0, st, vals, Lp, thr, dom.shard, parent, n_pass);
    });
    return pc_launch_check(what);
}

// fparent: [n_foreign][n], every value in [0, n) (a forest k_cc_union left: I1)
int pc_launch_cc_merge(int32_t* parent, const int32_t* fparent, int n_foreign, int n, hipStream_t st) {
    if (n_foreign <= 0 || n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_cc_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, parent, fparent, n_foreign, n);
    return pc_launch_check("k_cc_merge");
}

// depth <= n - 1 before; ceil(log2 n) halvings leave depth <= 1, and the last round's labels read two levels up: the root
int pc_launch_cc_labels(int32_t* parent, int32_t* labels, int n, hipStream_t st) {
    if (n <= 0) return PC_OK;
    int rounds = 1;
    while ((1 << rounds) < n && rounds < 31) ++rounds;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_cc_labels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, parent, labels, n);
        const int rc = pc_launch_check("k_cc_labels");
        if (rc != PC_OK) return rc;
    }
    return PC_OK;
}
