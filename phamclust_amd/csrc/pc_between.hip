// pc_between.hip -- the kernels of pc_fill_between: for a partition of the genomes into G groups, the G x G table of the count, sum,
// minimum and maximum of the pair values between every two groups (and within each group on the diagonal).  A value enters as its
// millionths, micro = rint(v * 1e6), an integer in [0, 10^6]: the sums, minima and maxima are integers, so the table is the same
// whatever the slab cut, the number of devices or the order of any atomic.
//   k_between_rows      one pass over a filled triangular slab.  A workgroup takes ONE target row of the slab (owned[k] = t, the values
//                       of pairs (s, t), s < t, at lbase[k] + s) or one segment of PC_BETWEEN_SEGMENT elements of a long row, so all its
//                       elements share a = group[t].  It accumulates over b = group[s] (consecutive int32 loads) in a table of G entries
//                       in LDS -- cnt << 40 | sum in one 64-bit word (a segment's sum is below 2^40, its count below 2^24), lo, hi -- and
//                       at the end adds the entries it touched into row a of the resident accumulator: consecutive b from consecutive
//                       lanes, so a wave's atomics cover contiguous bytes of one row.  Row starts are odd as often as even: a thread's
//                       two elements come by one 16-byte load where both lie in the segment and the pair is aligned (the slab's base is
//                       an allocation's, so an even index is), else by scalar loads of those that do; nothing is read outside
//                       [lbase[k], lbase[k + 1]).
//   k_between_qrows     the rows form (pc_fill_rows_between): one pass over a filled ROWS slab, f64[m][N], row r the values of query genome
//                       q = rows[r] to every genome g.  Grid (m, segments of a row); a workgroup takes one segment of one row, so its
//                       elements share a = group[q] (a < 0: the workgroup returns, an unlabelled query is in no pair).  An element is
//                       LIVE when g != q, group[g] >= 0 and (g > q or g is no query): a pair of two queries stands in two rows and the
//                       smaller genome's row takes it.  A dead element's value is never looked at -- not added, not checked -- so the
//                       diagonal and the dead duplicates may hold anything and a refused value is counted once per pair.  Same LDS
//                       table, same load rule (row r starts at r N, odd as often as even; nothing is read outside the row's segment),
//                       same wave reduction and flush into row a: bt_micro, bt_lds_add, bt_wave_add and bt_flush are the shared steps.
//                       k_between_rows keeps its own text of the loop: hoisting it into a body both kernels instantiate changed the
//                       triangular pass's register allocation and instruction order, and that kernel's device code is to stay as it is.
//   k_between_merge     several devices: the accumulators the other devices shipped added into the root's, entry by entry
//   k_between_fold      after the last slab: out[a][b] = acc[a][b] + acc[b][a] for a != b (sum and count added, minimum and maximum
//                       taken), the diagonal as it is; an entry no pair fell into reads cnt = 0, sum = 0, lo = INT32_MAX, hi = -1.
//                       The slabs are always filled as DISTANCES; a similarity table is the distance table inverted here -- sum' =
//                       cnt * 10^6 - sum, lo' = 10^6 - hi, hi' = 10^6 - lo -- which is what SymMatrix.invert() makes of a distance
//                       matrix (round(1 - d, 6) of a millionth is its complement) and so what every similarity the pipeline writes is.
//                       A similarity FILL rounds 1 - d and d separately, and at a decimal tie both round up: its millionths are not
//                       always the complements, and a table of them would not be the inverted distance table
// The accumulator stays on the device from the first slab to the last; nothing is read back per slab.
// What is atomic and why.  In LDS: ds atomics (64-bit add, 32-bit unsigned min / max) -- the lanes of a workgroup hit the same entry
// whenever two sources share a group.  A wave whose live lanes all name ONE group (one group in all, or a large group of neighbouring
// genomes) reduces its values by shuffles and issues the three atomics from one lane, instead of 64 that serialise on one address.
// In HBM: relaxed agent-scope atomics without a return value (64-bit add twice, 32-bit unsigned min / max) on the accumulator -- many
// workgroups share a row a, on every XCD, and the XCDs' L2s are not coherent with each other; adds and extremes commute, so no order
// matters.  No element issues a global atomic: a workgroup issues at most 4 G of them for up to 4,096 elements.  k_between_merge and
// k_between_fold run as launches of their own, after the passes: plain loads and stores, every thread its own entries.
// Progress: no workgroup ever waits for another; no flag is spun on; nothing sleeps.  The loops are the segment's (bounded by
// PC_BETWEEN_SEGMENT), the table's (bounded by G) and the wave reduction (six steps).
// The pass checks what the integers rely on, as pc_tree_pair_key does -- micro lies in [0, 10^6] and pc_div_million(micro) == v (an f64
// compare, which is one of bits for everything but the two zeros: -0.0 is a zero, and pc_div_million(-0.0) is +0.0) -- and counts what
// fails it in the accumulator's violation word (such a value is added nowhere): the host answers a non-zero
// count with PC_ERR_DATA.
#include <climits>

#include "pc_slab_pass.h"

#define BT_THREADS 256
#define BT_CNT_SHIFT 40
#define BT_SUM_MASK ((1ull << BT_CNT_SHIFT) - 1ull)
static_assert((unsigned long long)PC_BETWEEN_SEGMENT * 1000000ull < (1ull << BT_CNT_SHIFT), "a segment's sum must stay below the count field");
static_assert(PC_BETWEEN_SEGMENT % (2 * BT_THREADS) == 0, "a segment is whole iterations of the workgroup");
static_assert((size_t)PC_BETWEEN_MAX_GROUPS * 16 <= 65536, "the LDS table of the largest G");

// one value as its contribution: false (and one violation) when it is no millionth in [0, 1]
__device__ __forceinline__ bool bt_micro(double v, uint32_t& micro, uint32_t& bad) {
    const double k = __builtin_rint(v * 1.0e6);
    if (!(k >= 0.0 && k <= 1.0e6) || pc_div_million(k) != v) { ++bad; return false; }
    micro = (uint32_t)k;
    return true;
}

__device__ __forceinline__ void bt_lds_add(unsigned long long* t_sc, uint32_t* t_lo, uint32_t* t_hi, int b, unsigned long long sc, uint32_t lo, uint32_t hi) {
    atomicAdd(t_sc + b, sc);
    atomicMin(t_lo + b, lo);
    atomicMax(t_hi + b, hi);
}

// a lane's two elements (b0 / b1: their groups, -1: none; m0 / m1: their millionths) into the LDS table: one contribution where they
// share a group; a wave whose live lanes all name ONE group reduces by shuffles and one lane adds.  Wave-uniform: every lane of the wave calls it.
__device__ __forceinline__ void bt_wave_add(unsigned long long* t_sc, uint32_t* t_lo, uint32_t* t_hi, int lane, int b0, int b1, uint32_t m0, uint32_t m1) {
    const bool split = b0 >= 0 && b1 >= 0 && b0 != b1;
    int b = b0 >= 0 ? b0 : b1;
    unsigned long long sc = 0ull;
    uint32_t lo = ~0u, hi = 0u;
    if (b0 >= 0) { sc = (1ull << BT_CNT_SHIFT) | m0; lo = hi = m0; }
    if (b1 >= 0 && !split) { sc += (1ull << BT_CNT_SHIFT) | m1; lo = m1 < lo ? m1 : lo; hi = m1 > hi ? m1 : hi; }
    const unsigned long long live = __ballot(b >= 0);
    if (live == 0ull) return;                      // (the whole wave)
    const int leader = __ffsll((long long)live) - 1;
    const int lb = __shfl(b, leader);
    if (!__any(split || (b >= 0 && b != lb))) {
        // one group for the whole wave: reduce, one lane adds
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            sc += __shfl_xor(sc, off);
            const uint32_t ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
            lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
        }
        if (lane == leader) bt_lds_add(t_sc, t_lo, t_hi, lb, sc, lo, hi);
    } else {
        if (b >= 0) bt_lds_add(t_sc, t_lo, t_hi, b, sc, lo, hi);
        if (split) bt_lds_add(t_sc, t_lo, t_hi, b1, (1ull << BT_CNT_SHIFT) | m1, m1, m1);
    }
}

// the entries of the LDS table the segment touched into row a of the resident accumulator, and the segment's violations
__device__ __forceinline__ void bt_flush(const unsigned long long* t_sc, const uint32_t* t_lo, const uint32_t* t_hi, int a, int G, int tid, uint32_t bad,
                                         PcBetweenAcc acc) {
    __syncthreads();
    const size_t row = (size_t)a * (size_t)G;
    for (int b = tid; b < G; b += BT_THREADS) {
        const unsigned long long sc = t_sc[b];
        if (sc == 0ull) continue;                      // (no element of this segment in group b; a counted element sets the count field)
        (void)__hip_atomic_fetch_add(acc.sum + row + b, sc & BT_SUM_MASK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(acc.cnt + row + b, sc >> BT_CNT_SHIFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_min(acc.lo + row + b, t_lo[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(acc.hi + row + b, t_hi[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (bad) (void)__hip_atomic_fetch_add(acc.bad, (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(BT_THREADS) void k_between_rows(const double* __restrict__ vals, PcShard sh, const int32_t* __restrict__ group, int G,
                                                            PcBetweenAcc acc) {
    extern __shared__ unsigned long long bt_table[];
    unsigned long long* const t_sc = bt_table;
    uint32_t* const t_lo = (uint32_t*)(bt_table + G);
    uint32_t* const t_hi = t_lo + G;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int64_t r0 = sh.lbase[k], len = sh.lbase[k + 1] - r0, s0 = (int64_t)blockIdx.y * PC_BETWEEN_SEGMENT;
    if (s0 >= len) return;                             // (the whole workgroup: a row shorter than this segment's start)
    const int64_t e0 = r0 + s0, e1 = r0 + (len - s0 < PC_BETWEEN_SEGMENT ? len : s0 + PC_BETWEEN_SEGMENT);
    const int a = group[sh.ident ? k : sh.owned[k]];
    if ((unsigned)a >= (unsigned)G) return;            // (the whole workgroup; the host has checked the labels: never)
    for (int b = tid; b < G; b += BT_THREADS) { t_sc[b] = 0ull; t_lo[b] = ~0u; t_hi[b] = 0u; }
    __syncthreads();
    uint32_t bad = 0;
#pragma unroll 1
    for (int64_t base = e0 & ~(int64_t)1; base < e1; base += 2 * BT_THREADS) {       // (wave-uniform: the reduction below is the wave's)
        const int64_t i = base + 2 * tid;
        const bool h0 = i >= e0 && i < e1, h1 = i + 1 < e1;                             // (i + 1 > e0 always: base >= e0 - 1)
        double v0 = 0.0, v1 = 0.0;
        if (h0 && h1) { const double2 v = *reinterpret_cast<const double2*>(vals + i); v0 = v.x; v1 = v.y; }
        else if (h0) v0 = vals[i];
        else if (h1) v1 = vals[i + 1];
        uint32_t m0 = 0, m1 = 0;
        int b0 = -1, b1 = -1;
        if (h0 && bt_micro(v0, m0, bad)) b0 = group[i - r0];
        if (h1 && bt_micro(v1, m1, bad)) b1 = group[i + 1 - r0];
        if ((unsigned)b0 >= (unsigned)G && b0 != -1) { ++bad; b0 = -1; }                // (the host has checked the labels: never)
        if ((unsigned)b1 >= (unsigned)G && b1 != -1) { ++bad; b1 = -1; }
        // the lane's two elements as one contribution where they share a group
        const bool split = b0 >= 0 && b1 >= 0 && b0 != b1;
        int b = b0 >= 0 ? b0 : b1;
        unsigned long long sc = 0ull;
        uint32_t lo = ~0u, hi = 0u;
        if (b0 >= 0) { sc = (1ull << BT_CNT_SHIFT) | m0; lo = hi = m0; }
        if (b1 >= 0 && !split) { sc += (1ull << BT_CNT_SHIFT) | m1; lo = m1 < lo ? m1 : lo; hi = m1 > hi ? m1 : hi; }
        const unsigned long long live = __ballot(b >= 0);
        if (live == 0ull) continue;                    // (the whole wave)
        const int leader = __ffsll((long long)live) - 1;
        const int lb = __shfl(b, leader);
        if (!__any(split || (b >= 0 && b != lb))) {
            // one group for the whole wave: reduce, one lane adds
#pragma unroll
            for (int off = 32; off; off >>= 1) {
                sc += __shfl_xor(sc, off);
                const uint32_t ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
                lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
            }
            if (lane == leader) bt_lds_add(t_sc, t_lo, t_hi, lb, sc, lo, hi);
        } else {
            if (b >= 0) bt_lds_add(t_sc, t_lo, t_hi, b, sc, lo, hi);
            if (split) bt_lds_add(t_sc, t_lo, t_hi, b1, (1ull << BT_CNT_SHIFT) | m1, m1, m1);
        }
    }
    __syncthreads();
    const size_t row = (size_t)a * (size_t)G;
    for (int b = tid; b < G; b += BT_THREADS) {
        const unsigned long long sc = t_sc[b];
        if (sc == 0ull) continue;                      // (no element of this segment in group b; a counted element sets the count field)
        (void)__hip_atomic_fetch_add(acc.sum + row + b, sc & BT_SUM_MASK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(acc.cnt + row + b, sc >> BT_CNT_SHIFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_min(acc.lo + row + b, t_lo[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(acc.hi + row + b, t_hi[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (bad) (void)__hip_atomic_fetch_add(acc.bad, (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// element g of query genome q's row is a pair of the table: PcRowsDomain::live's rule (the diagonal is no pair; a pair of two queries
// stands in two rows and is the smaller one's), and a member of no group is in no pair
__device__ __forceinline__ bool bt_qlive(const PcRowsSlab& d, const int32_t* __restrict__ group, int q, int64_t g) {
    return g != q && group[g] >= 0 && (g > q || !d.is_query[g]);
}

// the rows form: grid (m, segments of a row of n); a workgroup takes one segment of one query row
__global__ __launch_bounds__(BT_THREADS) void k_between_qrows(const double* __restrict__ vals, PcRowsSlab d, const int32_t* __restrict__ group, int G,
                                                             PcBetweenAcc acc) {
    extern __shared__ unsigned long long bt_table[];
    unsigned long long* const t_sc = bt_table;
    uint32_t* const t_lo = (uint32_t*)(bt_table + G);
    uint32_t* const t_hi = t_lo + G;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int64_t len = d.n, r0 = (int64_t)k * len, s0 = (int64_t)blockIdx.y * PC_BETWEEN_SEGMENT;
    if (s0 >= len) return;                             // (the whole workgroup; the grid is cut to the row: never)
    const int64_t e0 = r0 + s0, e1 = r0 + (len - s0 < PC_BETWEEN_SEGMENT ? len : s0 + PC_BETWEEN_SEGMENT);
    const int q = d.rows[k], a = group[q];
    if ((unsigned)a >= (unsigned)G) return;            // (the whole workgroup: an unlabelled query is in no pair of the table)
    for (int b = tid; b < G; b += BT_THREADS) { t_sc[b] = 0ull; t_lo[b] = ~0u; t_hi[b] = 0u; }
    __syncthreads();
    uint32_t bad = 0;
#pragma unroll 1
    for (int64_t base = e0 & ~(int64_t)1; base < e1; base += 2 * BT_THREADS) {       // (wave-uniform: the reduction below is the wave's)
        const int64_t i = base + 2 * tid;
        const bool h0 = i >= e0 && i < e1, h1 = i + 1 < e1;                             // (i + 1 > e0 always: base >= e0 - 1)
        double v0 = 0.0, v1 = 0.0;
        if (h0 && h1) { const double2 v = *reinterpret_cast<const double2*>(vals + i); v0 = v.x; v1 = v.y; }
        else if (h0) v0 = vals[i];
        else if (h1) v1 = vals[i + 1];
        uint32_t m0 = 0, m1 = 0;
        int b0 = -1, b1 = -1;
        if (h0 && bt_qlive(d, group, q, i - r0) && bt_micro(v0, m0, bad)) b0 = group[i - r0];   // (a dead element's value is never looked at)
        if (h1 && bt_qlive(d, group, q, i + 1 - r0) && bt_micro(v1, m1, bad)) b1 = group[i + 1 - r0];
        if ((unsigned)b0 >= (unsigned)G && b0 != -1) { ++bad; b0 = -1; }                // (the host has checked the labels: never)
        if ((unsigned)b1 >= (unsigned)G && b1 != -1) { ++bad; b1 = -1; }
        bt_wave_add(t_sc, t_lo, t_hi, lane, b0, b1, m0, m1);
    }
    bt_flush(t_sc, t_lo, t_hi, a, G, tid, bad, acc);
}

// staged: n_foreign accumulators of `bytes` each
__global__ __launch_bounds__(256) void k_between_merge(PcBetweenAcc acc, const char* __restrict__ staged, size_t bytes, int n_foreign, int G) {
    const size_t gg = (size_t)G * (size_t)G, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= gg) return;
    unsigned long long sum = acc.sum[idx], cnt = acc.cnt[idx], bad = 0ull;
    uint32_t lo = acc.lo[idx], hi = acc.hi[idx];
    for (int f = 0; f < n_foreign; ++f) {
        const PcBetweenAcc o = pc_between_view((void*)(staged + (size_t)f * bytes), G);
        sum += o.sum[idx]; cnt += o.cnt[idx];
        const uint32_t ol = o.lo[idx], oh = o.hi[idx];
        lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
        if (idx == 0) bad += *o.bad;
    }
    acc.sum[idx] = sum; acc.cnt[idx] = cnt; acc.lo[idx] = lo; acc.hi[idx] = hi;
    if (idx == 0) *acc.bad += bad;
}

__global__ __launch_bounds__(256) void k_between_fold(PcBetweenAcc acc, long long* __restrict__ out_sum, long long* __restrict__ out_cnt,
                                                      int32_t* __restrict__ out_lo, int32_t* __restrict__ out_hi, unsigned long long* __restrict__ out_bad, int G,
                                                      int invert) {
    const size_t gg = (size_t)G * (size_t)G, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= gg) return;
    const size_t a = idx / (size_t)G, b = idx - a * (size_t)G, mirror = b * (size_t)G + a;
    unsigned long long sum = acc.sum[idx], cnt = acc.cnt[idx];
    uint32_t lo = acc.lo[idx], hi = acc.hi[idx];
    if (a != b) {
        sum += acc.sum[mirror]; cnt += acc.cnt[mirror];
        const uint32_t ol = acc.lo[mirror], oh = acc.hi[mirror];
        lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
    }
    if (invert && cnt) {                               // (lo <= hi <= 10^6 and sum <= cnt * 10^6: the pass admits nothing else)
        sum = cnt * 1000000ull - sum;
        const uint32_t l = 1000000u - hi;
        hi = 1000000u - lo; lo = l;
    }
    out_sum[idx] = (long long)sum; out_cnt[idx] = (long long)cnt;
    out_lo[idx] = cnt ? (int32_t)lo : INT32_MAX; out_hi[idx] = cnt ? (int32_t)hi : -1;
    if (idx == 0) *out_bad = *acc.bad;
}

static bool between_groups_ok(int G, const char* what) {
    if (G >= 1 && G <= PC_BETWEEN_MAX_GROUPS) return true;
    pc_set_error("%s: %d groups (1 .. PC_BETWEEN_MAX_GROUPS = %d)", what, G, PC_BETWEEN_MAX_GROUPS);
    return false;
}
static dim3 between_grid(int G) { return dim3((unsigned)(((size_t)G * (size_t)G + 255) / 256)); }

int pc_launch_between_init(void* acc, int G, hipStream_t st) {
    if (!between_groups_ok(G, "pc_launch_between_init")) return PC_ERR_ARG;
    const PcBetweenAcc v = pc_between_view(acc, G);
    PC_HIP(hipMemsetAsync(acc, 0, pc_between_bytes(G), st));
    PC_HIP(hipMemsetAsync(v.lo, 0xff, (size_t)G * (size_t)G * 4, st));
    return PC_OK;
}

int pc_launch_between_rows(const double* vals, int64_t Lp, const PcShard& sh, int64_t max_row, const int32_t* group, int G, void* acc, hipStream_t st) {
    if (Lp <= 0 || sh.nown <= 0) return PC_OK;
    if (!between_groups_ok(G, "k_between_rows")) return PC_ERR_ARG;
    const int64_t segs = (std::max<int64_t>(max_row, 1) + PC_BETWEEN_SEGMENT - 1) / PC_BETWEEN_SEGMENT;
    if (max_row > Lp || segs > 65535) { pc_set_error("k_between_rows: a longest row of %lld in a slab of %lld values", (long long)max_row, (long long)Lp); return PC_ERR_ARG; }
    const dim3 grid((unsigned)sh.nown, (unsigned)segs), block(BT_THREADS);
    hipLaunchKernelGGL(k_between_rows, grid, block, (size_t)G * 16, st, vals, sh, group, G, pc_between_view(acc, G));
    return pc_launch_check("k_between_rows");
}

int pc_launch_between_qrows(const double* vals, int64_t Lp, const PcRowsSlab& dom, const int32_t* group, int G, void* acc, hipStream_t st) {
    if (!between_groups_ok(G, "k_between_qrows")) return PC_ERR_ARG;
    if (dom.n <= 0 || dom.m <= 0 || Lp != (int64_t)dom.m * dom.n) { pc_set_error("k_between_qrows: a rows slab of %d x %d is not %lld values", dom.m, dom.n, (long long)Lp); return PC_ERR_ARG; }
    const int64_t segs = ((int64_t)dom.n + PC_BETWEEN_SEGMENT - 1) / PC_BETWEEN_SEGMENT;
    if (segs > 65535) { pc_set_error("k_between_qrows: rows of %d values", dom.n); return PC_ERR_ARG; }
    const dim3 grid((unsigned)dom.m, (unsigned)segs), block(BT_THREADS);
    hipLaunchKernelGGL(k_between_qrows, grid, block, (size_t)G * 16, st, vals, dom, group, G, pc_between_view(acc, G));
    return pc_launch_check("k_between_qrows");
}

int pc_launch_between_merge(void* acc, const void* staged, int n_foreign, int G, hipStream_t st) {
    if (n_foreign <= 0) return PC_OK;
    if (!between_groups_ok(G, "k_between_merge")) return PC_ERR_ARG;
    hipLaunchKernelGGL(k_between_merge, between_grid(G), dim3(256), 0, st, pc_between_view(acc, G), (const char*)staged, pc_between_bytes(G), n_foreign, G);
    return pc_launch_check("k_between_merge");
}

int pc_launch_between_fold(const void* acc, void* out, int G, int invert, hipStream_t st) {
    if (!between_groups_ok(G, "k_between_fold")) return PC_ERR_ARG;
    const PcBetweenAcc o = pc_between_view(out, G);
    hipLaunchKernelGGL(k_between_fold, between_grid(G), dim3(256), 0, st, pc_between_view((void*)acc, G), (long long*)o.sum, (long long*)o.cnt,
                       (int32_t*)o.lo, (int32_t*)o.hi, o.bad, G, invert ? 1 : 0);
    return pc_launch_check("k_between_fold");
}
