// pc_slab_pass.h -- what a pass over a filled slab is, for the four units that hold one (pc_edges: count and emit, pc_components:
// union, pc_tree: the scan, pc_hist: the histogram).  A pass sees the slab as one flat f64[Lp] cut into chunks of SLAB_CHUNK elements, one workgroup each; a
// thread takes two consecutive elements (one 16-byte load) per iteration.  Which PAIR an element is, and whether it is one at all, is
// the DOMAIN's business -- every pass body is a template over it, written once:
//   PcTriDomain    a triangular slab, the shard layout a fill writes with condensed = 0: the values of pairs (s, owned[k]),
//                  s = 0 .. owned[k] - 1, at lbase[k] + s.  Every element is a pair.
//   PcRowsDomain   a rows slab (PcRowsSlab, pc_common.h): f64[m][n], element i the pair {rows[i / n], i % n}, LIVE or not.
// A domain is a value the kernel wrapper builds from its argument, with a per-thread Cursor beside it:
//   locate(i0)             what says where the workgroup's first element lies: ONE thread computes it, the others take it from LDS
//   start(origin)          the cursor of this thread's first iteration
//   live(at, i)            element i -- the thread's even element of this iteration, or the odd one behind it -- is a pair of the call
//   pair(at, i, a, b)      that pair's two genomes: a on the side a wave's 128 consecutive elements mostly share (the target of a
//                          triangular slab, the query genome of a rows slab), b the other; elements are asked in ascending order
//   sorted(a, b, s, t)     (static) the same pair as source s < target t, for the passes that need the order
//   step(at)               on to the next iteration, SLAB_STRIDE elements further
//   kLocateFirst           the domain filters on liveness, so it is located ahead of the loads (a barrier of its own); a domain that
//                          does not is located behind them, on the barrier a body has anyway, and only where pairs are named
// Internal; everything here is static or inline.
#pragma once
#include "pc_pairs.h"

#define SLAB_THREADS 256
#define SLAB_ITERS 8
#define SLAB_STRIDE (SLAB_THREADS * 2)                 // elements the workgroup reads per iteration: two consecutive ones per thread
#define SLAB_CHUNK (SLAB_STRIDE * SLAB_ITERS)          // 4,096 elements = 32 KB of slab per workgroup

// elements i and i + 1 of the slab (i even: the slab's base is an allocation's, chunks and thread slots are even, so the 16-byte
// load is aligned); the last element of an odd Lp is loaded alone, nothing is read beyond Lp.  Returns how many of the two exist.
__device__ __forceinline__ int pc_slab_load(const double* __restrict__ vals, int64_t i, int64_t Lp, double& a, double& b) {
    a = b = 0.0;
    if (i + 1 < Lp) {
        const double2 v = *reinterpret_cast<const double2*>(vals + i);
        a = v.x; b = v.y;
        return 2;
    }
    if (i < Lp) { a = vals[i]; return 1; }
    return 0;
}

struct PcTriDomain {
    static constexpr bool kLocateFirst = false;
    typedef int Origin;                                // the row k of the chunk's first element
    struct Cursor { int k; };                          // the row reached so far
    PcShard sh;
    // lbase[k] <= i0 < lbase[k + 1] (lbase[0] = 0 <= i0 < Lp = lbase[nown]); rows of length 0 repeat an lbase value and can never be
    // the answer
    __device__ __forceinline__ Origin locate(int64_t i0) const {
        int lo = 0, hi = sh.nown;
        while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (sh.lbase[mid] <= i0) lo = mid; else hi = mid; }
        return lo;
    }
    __device__ __forceinline__ Cursor start(Origin k_first) const { return Cursor{k_first}; }
    __device__ __forceinline__ bool live(const Cursor&, int64_t) const { return true; }
    // the forward walk over empty and short rows (an element that exists lies below Lp = lbase[nown]: it stops at k + 1 <= nown)
    __device__ __forceinline__ void pair(Cursor& at, int64_t i, int& a, int& b) const {
        int k = at.k;                                  // (a local: the walk then compiles to one loop, no second load of lbase[k + 1])
        while (i >= sh.lbase[k + 1]) ++k;
        at.k = k;
        b = (int)(i - sh.lbase[k]); a = sh.owned[k];
    }
    static __device__ __forceinline__ void sorted(int a, int b, int& s, int& t) { s = b; t = a; }       // (b < a by the layout)
    __device__ __forceinline__ void step(Cursor&) const {}
};

// (row, column) of a thread's elements in a rows slab without a division per value: the workgroup's first element by ONE 64-bit
// division, a thread's first by one 32-bit division, every further iteration by two adds and a carry (adv_* = SLAB_STRIDE / n and
// SLAB_STRIDE % n, set by pc_slab_domain_check).  An element that exists lies below Lp = m * n: its row is one of the slab's.
struct PcRowsDomain {
    static constexpr bool kLocateFirst = true;
    typedef int2 Origin;                               // (row, column) of the chunk's first element
    struct Cursor { int row, col; };                   // of the thread's even element; its odd one follows
    PcRowsSlab d;
    __device__ __forceinline__ Origin locate(int64_t i0) const { const int64_t r = i0 / d.n; return make_int2((int)r, (int)(i0 - r * d.n)); }
    __device__ __forceinline__ Cursor start(Origin origin) const {
        const uint32_t x = (uint32_t)origin.y + threadIdx.x * 2u, r = x / (uint32_t)d.n;      // (the thread's offset in the chunk < 2^16)
        return Cursor{origin.x + (int)r, (int)(x - r * (uint32_t)d.n)};
    }
    // (live and pair each work the odd element's place out, and read rows[] for it, where they are asked: deliberately -- nothing of
    // it is then kept in registers across a body's barrier, and the second computation is a compare and two selects)
    __device__ __forceinline__ Cursor element(const Cursor& at, int64_t i) const {
        if (!(i & 1)) return at;                       // (chunks and thread slots are even: the even element has an even index)
        const bool wrap = at.col + 1 == d.n;
        return Cursor{at.row + (wrap ? 1 : 0), wrap ? 0 : at.col + 1};
    }
    // element (row, g) with query genome q = rows[row]: the diagonal is no pair, and a pair of two query genomes is taken once, in
    // the row of the smaller one
    __device__ __forceinline__ bool live(const Cursor& at, int64_t i) const {
        const Cursor e = element(at, i);
        const int q = d.rows[e.row], g = e.col;
        return g > q || (g < q && !d.is_query[g]);
    }
    // (a wave's elements lie mostly in ONE row: they share the query genome, whichever end of the pair it is)
    __device__ __forceinline__ void pair(Cursor& at, int64_t i, int& a, int& b) const {
        const Cursor e = element(at, i);
        a = d.rows[e.row]; b = e.col;
    }
    static __device__ __forceinline__ void sorted(int a, int b, int& s, int& t) { s = a < b ? a : b; t = a < b ? b : a; }
    __device__ __forceinline__ void step(Cursor& at) const {
        at.row += d.adv_rows; at.col += d.adv_cols;
        if (at.col >= d.n) { at.col -= d.n; ++at.row; }
    }
};

// one thread locates the workgroup's chunk for all (the caller's barrier hands `origin`, a word of LDS, on)
template <class Dom> __device__ __forceinline__ void pc_slab_locate(const Dom& dom, typename Dom::Origin& origin) {
    if (threadIdx.x == 0) origin = dom.locate((int64_t)blockIdx.x * SLAB_CHUNK);
}

// ---- host: what every launcher of a pass does around its launch ----
// a rows domain must cover the slab, and gets the stride between a thread's iterations; `what`: the kernel, for the message texts
static int pc_slab_domain_check(PcSlabDomain& dom, int64_t Lp, const char* what) {
    if (!dom.is_rows) return PC_OK;
    PcRowsSlab& r = dom.rows;
    if (r.n <= 0 || r.m <= 0 || Lp != (int64_t)r.m * r.n) { pc_set_error("%s: a rows slab of %d x %d is not %lld values", what, r.m, r.n, (long long)Lp); return PC_ERR_ARG; }
    r.adv_rows = SLAB_STRIDE / r.n; r.adv_cols = SLAB_STRIDE % r.n;
    return PC_OK;
}
static int pc_launch_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("%s launch: %s", what, hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
