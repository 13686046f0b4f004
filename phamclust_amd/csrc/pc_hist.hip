// pc_hist.hip -- the kernels of pc_fill_hist: the exact histogram of every pair value of the collection.  A delivered value is
// round(x, 6), one of the 10^6 + 1 millionths in [0, 1] (micro = rint(v * 1e6), checked as bt_micro of pc_between.hip checks it), so the
// whole distribution is PC_HIST_BINS = 1,000,001 integer bins -- one such array per CLASS: one class without a partition; with one,
// class 0 the pairs whose two genomes share a group ("within"), class 1 the others ("between").  The resident state is
// u64 hist[classes][PC_HIST_BINS] and the 8-byte count of values that are no millionth behind it (pc_hist_bytes, pc_common.h): cleared
// once per call, on the device from the first slab to the last, nothing read back per slab.  Integers: the histogram is the same whatever
// the slab cut, the number of devices or the order of any atomic.
//   k_hist_pass / k_hist_pass_rows   ONE body, pc_hist_body, under two kernels per form (with / without a partition): over a triangular
//                       slab (PcTriDomain) and over a rows slab (PcRowsDomain; pc_fill_rows_hist).  It streams the slab as every slab
//                       pass does (pc_slab_pass.h: flat f64[Lp], chunks of SLAB_CHUNK = 4,096 elements, 256 threads, eight 16-byte
//                       loads per thread, the odd last element alone, nothing read beyond Lp) and asks the domain which elements are
//                       pairs (a dead element's value is never looked at: not binned, not checked) and, with a partition, which two
//                       genomes a pair joins: class = group[a] != group[b].  Without a partition no label is loaded and no pair named.
//                       A live element is the 21-bit key  class << 20 | micro.  The workgroup counts its chunk's keys in an
//                       open-addressing table in LDS -- PC_HIST_SLOTS = 2,048 slots, a key word and a u32 count word each, 16 KiB: nine
//                       workgroups of it fit a CU's 160 KiB -- and flushes the occupied slots at the end of the chunk.
//                         slot     pc_hist_slot(key) = (key * 2654435761) >> 21 (the top 11 bits of the product), then linear probing,
//                                  at most PC_HIST_PROBES = 8 slots; the key word is claimed by compare-and-swap against the empty
//                                  marker ~0u, which is no key (0 IS one: micro 0 of class 0), the count word takes a ds add
//                         overflow an insert that finds its 8 slots held by other keys adds to the global bin itself (a chunk of
//                                  4,096 all-distinct aai / peq values holds more keys than the table has slots: privatising buys
//                                  nothing there, and loses nothing)
//                         peel     ahead of the LDS atomics, PC_HIST_PEEL = 2 rounds per element slot: the wave reads its first live
//                                  lane's key, ballots the lanes that hold the same, ONE lane adds the popcount, those lanes retire.
//                                  Set-metric values are a few hundred ratios and d = 1.0 alone a fifth of all pairs: without the peel
//                                  64 lanes of one value serialise on one LDS address (bt_wave_add's single-group path is the precedent)
//                         flush    after a barrier, every occupied slot: one 64-bit add into hist; the violations once per workgroup
//   k_hist_merge        several devices: the states the other devices shipped added into the root's, word by word (the violation word
//                       is the last word of a state)
//   k_hist_finish       after the last slab: the state into the result buffer, as_distance == 0 with every class reversed (bin k <->
//                       10^6 - k: the slabs are always filled as DISTANCES and a similarity histogram is the inverted matrix's, the
//                       complement of every millionth, as pc_fill_between's table -- not a similarity fill's values, which differ at a
//                       decimal tie).  The MOMENTS are left to the host: it receives the whole array anyway, Python integers hold the
//                       sums of k^3 (about 10^30 at N = 2^22) without a 128-bit emulation here, and the class totals are one host
//                       pass over the pinned array (pc_fill_hist's *n_pairs).
// What is atomic and why.  In LDS: ds compare-and-swap on a key word, ds add on a count word -- the lanes of a workgroup meet on a slot
// whenever two elements share a value.  In HBM: relaxed agent-scope 64-bit fetch_add without a return value on hist and on the violation
// word -- every workgroup, on every XCD, adds into the same bins and the XCDs' L2s are not coherent with each other; adds commute, so no
// order matters.  No element of a chunk that fits the table issues a global atomic: a workgroup issues at most one per occupied slot, and
// one more per insert that overflowed.  k_hist_merge and k_hist_finish run as launches of their own, after the passes: plain loads and
// stores, every thread its own words.
// Progress: no workgroup ever waits for another; no flag is spun on; nothing sleeps.  The loops are the chunk's (SLAB_ITERS), the peel's
// (PC_HIST_PEEL), the probe's (PC_HIST_PROBES) and the flush's (PC_HIST_SLOTS / 256): all bounded.
#include "pc_slab_pass.h"

#define PC_HIST_SLOTS 2048
#define PC_HIST_SLOT_BITS 11
#define PC_HIST_PROBES 8
#define PC_HIST_PEEL 2
#define PC_HIST_EMPTY (~0u)
#define PC_HIST_MICRO_BITS 20
static_assert((1 << PC_HIST_SLOT_BITS) == PC_HIST_SLOTS, "the slot is the top bits of the hash");
static_assert(PC_HIST_BINS <= (1 << PC_HIST_MICRO_BITS), "a millionth takes 20 bits of a key");
static_assert(PC_HIST_SLOTS % SLAB_THREADS == 0, "the table is cleared and flushed in whole rounds of the workgroup");
static_assert(PC_HIST_SLOTS < SLAB_CHUNK, "a chunk of distinct values overflows the table: the overflow path is a path of every aai / peq fill");

__host__ __device__ inline uint32_t pc_hist_slot(uint32_t key) { return (key * 2654435761u) >> (32 - PC_HIST_SLOT_BITS); }

// one value as its millionth: false (and one violation) when it is none in [0, 1] (bt_micro's check: -0.0 is the millionth 0)
__device__ __forceinline__ bool pc_hist_micro(double v, uint32_t& micro, uint32_t& bad) {
    const double k = __builtin_rint(v * 1.0e6);
    if (!(k >= 0.0 && k <= 1.0e6) || pc_div_million(k) != v) { ++bad; return false; }
    micro = (uint32_t)k;
    return true;
}

// n elements of `key` into the workgroup's table, or past it into the global bin
__device__ __forceinline__ void pc_hist_insert(uint32_t* t_key, uint32_t* t_cnt, uint32_t key, uint32_t n, unsigned long long* hist) {
    uint32_t slot = pc_hist_slot(key);
#pragma unroll 1
    for (int p = 0; p < PC_HIST_PROBES; ++p) {
        const uint32_t was = atomicCAS(t_key + slot, PC_HIST_EMPTY, key);
        if (was == PC_HIST_EMPTY || was == key) { atomicAdd(t_cnt + slot, n); return; }
        slot = (slot + 1) & (PC_HIST_SLOTS - 1);
    }
    const size_t bin = (size_t)(key >> PC_HIST_MICRO_BITS) * PC_HIST_BINS + (key & ((1u << PC_HIST_MICRO_BITS) - 1u));
    (void)__hip_atomic_fetch_add(hist + bin, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a lane's element (key, or PC_HIST_EMPTY: none) into the table: the wave's hot keys by one lane each, the rest lane by lane.
// Wave-uniform: every lane of the wave calls it.
__device__ __forceinline__ void pc_hist_wave_add(uint32_t* t_key, uint32_t* t_cnt, int lane, uint32_t key, unsigned long long* hist) {
    bool live = key != PC_HIST_EMPTY;
#pragma unroll
    for (int r = 0; r < PC_HIST_PEEL; ++r) {
        const unsigned long long mask = __ballot(live);
        if (mask == 0ull) return;                      // (the whole wave)
        const int leader = __ffsll((long long)mask) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)key, leader);
        const bool same = live && key == lk;
        const unsigned long long hot = __ballot(same);
        if (lane == leader) pc_hist_insert(t_key, t_cnt, lk, (uint32_t)__popcll(hot), hist);
        if (same) live = false;
    }
    if (live) pc_hist_insert(t_key, t_cnt, key, 1u, hist);
}

template <bool PART, class Dom>
__device__ __forceinline__ void pc_hist_body(const double* __restrict__ vals, int64_t Lp, const Dom dom, const int32_t* __restrict__ group,
                                             unsigned long long* hist, unsigned long long* n_bad) {
    __shared__ uint32_t t_key[PC_HIST_SLOTS];
    __shared__ uint32_t t_cnt[PC_HIST_SLOTS];
    __shared__ uint32_t wg_bad;
    __shared__ typename Dom::Origin origin;
    constexpr bool kLocate = Dom::kLocateFirst || PART;       // (a triangular slab without a partition names no pair: nothing to locate)
    const int tid = threadIdx.x, lane = tid & 63;
    for (int s = tid; s < PC_HIST_SLOTS; s += SLAB_THREADS) { t_key[s] = PC_HIST_EMPTY; t_cnt[s] = 0u; }
    if (tid == 0) wg_bad = 0u;
    if constexpr (kLocate) pc_slab_locate(dom, origin);
    __syncthreads();
    typename Dom::Cursor at{};
    if constexpr (kLocate) at = dom.start(origin);
    const int64_t base = (int64_t)blockIdx.x * SLAB_CHUNK + (int64_t)tid * 2;
    uint32_t key_a[SLAB_ITERS], key_b[SLAB_ITERS];
    uint32_t bad = 0;
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {
        double va, vb;
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, va, vb);
        uint32_t ka = PC_HIST_EMPTY, kb = PC_HIST_EMPTY, micro = 0;
        if (have > 0 && dom.live(at, i) && pc_hist_micro(va, micro, bad)) {     // (a dead element's value is never looked at)
            ka = micro;
            if constexpr (PART) { int a, b; dom.pair(at, i, a, b); ka |= (uint32_t)(group[a] != group[b]) << PC_HIST_MICRO_BITS; }
        }
        if (have > 1 && dom.live(at, i + 1) && pc_hist_micro(vb, micro, bad)) {
            kb = micro;
            if constexpr (PART) { int a, b; dom.pair(at, i + 1, a, b); kb |= (uint32_t)(group[a] != group[b]) << PC_HIST_MICRO_BITS; }
        }
        key_a[j] = ka; key_b[j] = kb;
        dom.step(at);
    }
#pragma unroll
    for (int j = 0; j < SLAB_ITERS; ++j) {              // (wave-uniform: the peel is the wave's)
        pc_hist_wave_add(t_key, t_cnt, lane, key_a[j], hist);
        pc_hist_wave_add(t_key, t_cnt, lane, key_b[j], hist);
    }
    if (bad) atomicAdd(&wg_bad, bad);
    __syncthreads();
    for (int s = tid; s < PC_HIST_SLOTS; s += SLAB_THREADS) {
        const uint32_t key = t_key[s];
        if (key == PC_HIST_EMPTY) continue;
        const size_t bin = (size_t)(key >> PC_HIST_MICRO_BITS) * PC_HIST_BINS + (key & ((1u << PC_HIST_MICRO_BITS) - 1u));
        (void)__hip_atomic_fetch_add(hist + bin, (unsigned long long)t_cnt[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid == 0 && wg_bad) (void)__hip_atomic_fetch_add(n_bad, (unsigned long long)wg_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool PART>
__global__ __launch_bounds__(SLAB_THREADS) void k_hist_pass(const double* __restrict__ vals, int64_t Lp, PcShard sh, const int32_t* __restrict__ group,
                                                            unsigned long long* hist, unsigned long long* n_bad) {
    pc_hist_body<PART>(vals, Lp, PcTriDomain{sh}, group, hist, n_bad);
}
template <bool PART>
__global__ __launch_bounds__(SLAB_THREADS) void k_hist_pass_rows(const double* __restrict__ vals, int64_t Lp, PcRowsSlab dom, const int32_t* __restrict__ group,
                                                                 unsigned long long* hist, unsigned long long* n_bad) {
    pc_hist_body<PART>(vals, Lp, PcRowsDomain{dom}, group, hist, n_bad);
}

// staged: n_foreign states of `words` 64-bit words each (the bins of every class, then the violation word)
__global__ __launch_bounds__(256) void k_hist_merge(unsigned long long* __restrict__ state, const unsigned long long* __restrict__ staged, size_t words,
                                                    int n_foreign) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    unsigned long long x = state[idx];
    for (int f = 0; f < n_foreign; ++f) x += staged[(size_t)f * words + idx];
    state[idx] = x;
}

__global__ __launch_bounds__(256) void k_hist_finish(const unsigned long long* __restrict__ state, long long* __restrict__ out, int classes, int invert) {
    const size_t words = (size_t)classes * PC_HIST_BINS + 1, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= words) return;
    if (idx + 1 == words || !invert) { out[idx] = (long long)state[idx]; return; }
    const size_t c = idx / PC_HIST_BINS, k = idx - c * PC_HIST_BINS;
    out[idx] = (long long)state[c * PC_HIST_BINS + (PC_HIST_BINS - 1 - k)];
}

int pc_hist_table_slot_count(void) { return PC_HIST_SLOTS; }
int pc_hist_probe_bound(void) { return PC_HIST_PROBES; }

static bool hist_classes_ok(int classes, const char* what) {
    if (classes == 1 || classes == 2) return true;
    pc_set_error("%s: %d classes (1 or 2)", what, classes);
    return false;
}
static dim3 hist_grid(int classes) { return dim3((unsigned)((pc_hist_bytes(classes) / 8 + 255) / 256)); }

int pc_launch_hist_pass(const double* vals, int64_t Lp, PcSlabDomain dom, const int32_t* group, int classes, void* state, hipStream_t st) {
    if (Lp <= 0) return PC_OK;
    const char* const what = dom.is_rows ? "k_hist_pass_rows" : "k_hist_pass";
    if (!hist_classes_ok(classes, what)) return PC_ERR_ARG;
    if ((classes == 2) != (group != nullptr)) { pc_set_error("%s: %d classes %s labels", what, classes, group ? "with" : "without"); return PC_ERR_ARG; }
    const int rc = pc_slab_domain_check(dom, Lp, what);
    if (rc != PC_OK) return rc;
    unsigned long long* const hist = (unsigned long long*)state;
    unsigned long long* const n_bad = hist + (size_t)classes * PC_HIST_BINS;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1>(group ? 1 : 0, [&](auto form) {
        constexpr bool PART = decltype(form)::value != 0;
        if (dom.is_rows) hipLaunchKernelGGL((k_hist_pass_rows<PART>), grid, block, 0, st, vals, Lp, dom.rows, group, hist, n_bad);
        else hipLaunchKernelGGL((k_hist_pass<PART>), grid, block, 0, st, vals, Lp, dom.shard, group, hist, n_bad);
    });
    return pc_launch_check(what);
}

int pc_launch_hist_merge(void* state, const void* staged, int n_foreign, int classes, hipStream_t st) {
    if (n_foreign <= 0) return PC_OK;
    if (!hist_classes_ok(classes, "k_hist_merge")) return PC_ERR_ARG;
    hipLaunchKernelGGL(k_hist_merge, hist_grid(classes), dim3(256), 0, st, (unsigned long long*)state, (const unsigned long long*)staged,
                       pc_hist_bytes(classes) / 8, n_foreign);
    return pc_launch_check("k_hist_merge");
}

int pc_launch_hist_finish(const void* state, void* out, int classes, int invert, hipStream_t st) {
    if (!hist_classes_ok(classes, "k_hist_finish")) return PC_ERR_ARG;
    hipLaunchKernelGGL(k_hist_finish, hist_grid(classes), dim3(256), 0, st, (const unsigned long long*)state, (long long*)out, classes, invert ? 1 : 0);
    return pc_launch_check("k_hist_finish");
}
