// pc_affinity.hip -- the kernels of pc_fill_affinity: for a partition of the genomes into G groups, the N x G table of the sum, minimum
// and maximum of the pair values between every genome g and every group b (over x in b, x != g), and what a caller needs of it per
// genome: its entry for its own group and the nearest other group by mean, by minimum and by maximum.  A value enters as its
// millionths, micro = rint(v * 1e6), an integer in [0, 10^6] (bt_micro's rule, stated in pc_between.hip): sums, minima and maxima are
// integers, so the table is the same whatever the slab cut, the number of devices or the launch order.  The count of an entry is not
// stored: it is size[b] - [group[g] == b].
// The resident table is T[N][G] of (u64 sum, u32 lo, u32 hi), 16 bytes per entry, with the 8-byte violation count behind it
// (pc_affinity_bytes); an entry nothing was added to is (0, ~0, 0).  A filled triangular slab holds, for target t = t0 + k, the values
// of (s, t), s < t, at lbase[k] + s; an element belongs to T[t][group[s]] and to T[s][group[t]], and the two go through two launches:
//   k_aff_rows     T[t][group[s]].  One workgroup takes ONE target row and loops over all of it, accumulating over b = group[s] in a
//                  G-entry table in LDS (ds atomics; a wave whose live lanes all name one group reduces by shuffles and one lane adds,
//                  as k_between_rows does), then adds the entries it touched into row t of T by plain loads and stores.
//   k_aff_cols     T[s][group[t]].  A WAVE owns a block of PC_AFFINITY_BLOCK consecutive sources, lanes across sources, and a range of
//                  groups (the ranges are cut on the host, balanced by member count, so that N / block source blocks of triangular,
//                  unequal length still fill the device).  It walks the slab's targets group by group through member[] (the genomes
//                  sorted by (group, index)) and goff[] (each group's run in it): a group's members inside [max(t0, s0 + 1), t1) are
//                  one contiguous run of its member list, found by binary search.  Per target one run of 8 x block contiguous bytes is
//                  read; a lane keeps (sum, lo, hi) of ONE group in registers and adds them into T[s][a] once per (source, group,
//                  slab).  A workgroup is four such waves with four group ranges; they share nothing.
//   k_aff_merge    several devices: the tables the other devices shipped combined into the root's entry by entry (sums added, the
//                  smaller lo, the larger hi: a pair lies in exactly one stretch)
//   k_aff_finish   after the last slab: a wave per genome scans its G entries and writes the O(N) result -- own (sum, lo, hi) and, by
//                  each of the three criteria, the nearest OTHER non-empty group with the value that made it nearest; ties go to the
//                  smaller group index; means are compared as sum_b * size_c against sum_c * size_b in 64-bit integers (below 2^63
//                  for N <= 2^22: size_b * size_c <= N^2 / 4), never in floating point.  With want_table the converted table (sum i64,
//                  lo / hi i32, an empty entry as 0 / INT32_MAX / -1) is written beside it.  The slabs are always filled as DISTANCES;
//                  a similarity result is the distance result with every reported value complemented here (the reason is written above
//                  k_between_fold), so the nearest groups are the same in both directions.
// Who writes what.  Within a launch every entry of T is written by exactly one wave: row t of k_aff_rows' grid belongs to the workgroup
// of target t; entry (s, a) of k_aff_cols to the wave whose source block holds s and whose group range holds a.  The two passes are
// separate launches on the fill's stream, so the read-modify-write of an entry is never concurrent with another.
// What is atomic and why.  In LDS: ds atomics in k_aff_rows -- the lanes of a workgroup hit the same entry whenever two sources share a
// group.  In HBM: only the violation count (a relaxed agent-scope add, once per wave of k_aff_rows that found any); the table needs none,
// as above.  Both passes see every element of a slab and both leave a refused value out, but only the row pass counts it: the count is
// the number of refused VALUES.
// Progress: no workgroup waits for another; no flag is spun on.  The loops are a row's (bounded by its length), the table's (G), a
// group's member run and two binary searches over it.
// What is read: a row pass reads [lbase[k], lbase[k + 1]) of its row; a column pass reads lbase[k] + s for s < min(t, the row's
// length); nothing beyond Lp.
//
// The rows form (pc_fill_rows_affinity): n_rows query genomes against the groups, over ROWS slabs (PcRowsSlab: f64[m][N], row r the values
// of query genome rows[r] to every genome).  A label may be -1 here: a member of no group.  The resident state is T[n_rows][G] (row k the
// query rows[k]) | gain[N] | the violation count (pc_common.h).
//   k_aff_qrows    T[k][group[s]] over every column s != q with a label: a workgroup per row of the slab, the LDS table and the wave
//                  reduction of k_aff_rows (af_lds_add).  The diagonal and the columns of unlabelled genomes are not read.
//   k_aff_qcols    gain[g] (want_gain only): what the slab's query genomes add to the own entry of an old labelled genome g.  A lane per
//                  column, a row's group wave-uniform, the value loaded only where a lane of the wave matches (ballot).
//   k_aff_qfinish  a wave per query row through k_aff_finish's body (af_finish_row) with a row indirection and an own group that may be
//                  -1; behind them a thread per genome converts gain[].
// Who writes what.  A query's row lies in exactly one slab: row r0 + r of T is written once, whole, by the workgroup of slab row r (plain
// stores, no read-modify-write).  gain[g] has one writer per launch -- the lane of column g -- and the slabs' launches follow each other
// on one stream.  What is atomic: ds atomics in LDS as in k_aff_rows; in HBM the violation count alone.  A refused value is left out by
// both passes and counted by the row pass once per PAIR: a pair of two labelled query genomes stands in two rows that both read it, and
// the row of the smaller counts it (PcRowsDomain::live's rule).  Progress: no workgroup waits for another; the loops are a row's N
// columns, the slab's m rows, the table's G.  What is read: row r of the slab at columns below N; nothing beyond m * N.
#include <climits>

#include "pc_slab_pass.h"

#define AF_THREADS 256
#define AF_WAVES (AF_THREADS / 64)
#define AF_UNROLL 8
static_assert(PC_AFFINITY_BLOCK == 64, "a column-pass wave's lanes are its sources");
static_assert((size_t)PC_BETWEEN_MAX_GROUPS * 16 <= 65536, "the LDS table of the largest G");

// one value as its contribution: false (and one violation) when it is no millionth in [0, 1] (bt_micro of pc_between.hip)
__device__ __forceinline__ bool af_micro(double v, uint32_t& micro, uint32_t& bad) {
    const double k = __builtin_rint(v * 1.0e6);
    if (!(k >= 0.0 && k <= 1.0e6) || pc_div_million(k) != v) { ++bad; return false; }
    micro = (uint32_t)k;
    return true;
}

// (sum, lo, hi) added into one entry of the table: a plain 16-byte load and store, the entry is this wave's
__device__ __forceinline__ void af_entry_add(PcAffinityEntry* __restrict__ e, unsigned long long sum, uint32_t lo, uint32_t hi) {
    PcAffinityEntry x = *e;
    x.sum += sum; x.lo = lo < x.lo ? lo : x.lo; x.hi = hi > x.hi ? hi : x.hi;
    *e = x;
}

__global__ __launch_bounds__(256) void k_aff_init(PcAffinityEntry* __restrict__ tab, size_t n_entries) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_entries) tab[i] = PcAffinityEntry{0ull, ~0u, 0u};
    if (i == 0) *(unsigned long long*)(tab + n_entries) = 0ull;
}

// One wave's step of a row pass (k_aff_rows, k_aff_qrows): lane's millionths m into entry b of the workgroup's LDS table, b == -1: this lane
// adds nothing.  Called by the whole wave.  A wave whose live lanes all name one group reduces by shuffles and one lane adds; otherwise a
// ds atomic per live lane.
__device__ __forceinline__ void af_lds_add(int b, uint32_t m, int lane, unsigned long long* t_sum, uint32_t* t_lo, uint32_t* t_hi) {
    const unsigned long long live = __ballot(b >= 0);
    if (live == 0ull) return;                          // (the whole wave)
    const int leader = __ffsll((long long)live) - 1;
    const int lb = __shfl(b, leader);
    if (!__any(b >= 0 && b != lb)) {
        // one group for the whole wave: reduce, one lane adds
        unsigned long long sum = b >= 0 ? m : 0ull;
        uint32_t lo = b >= 0 ? m : ~0u, hi = b >= 0 ? m : 0u;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            sum += __shfl_xor(sum, off);
            const uint32_t ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
            lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
        }
        if (lane == leader) { atomicAdd(t_sum + lb, sum); atomicMin(t_lo + lb, lo); atomicMax(t_hi + lb, hi); }
    } else if (b >= 0) {
        atomicAdd(t_sum + b, (unsigned long long)m); atomicMin(t_lo + b, m); atomicMax(t_hi + b, m);
    }
}

// row pass: workgroup k takes target t0 + k
__global__ __launch_bounds__(AF_THREADS) void k_aff_rows(const double* __restrict__ vals, PcShard sh, int t0, const int32_t* __restrict__ group, int G,
                                                        PcAffinityEntry* __restrict__ tab, unsigned long long* __restrict__ n_bad) {
    extern __shared__ unsigned long long af_table[];
    unsigned long long* const t_sum = af_table;
    uint32_t* const t_lo = (uint32_t*)(af_table + G);
    uint32_t* const t_hi = t_lo + G;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int t = t0 + k;
    const int64_t r0 = sh.lbase[k];
    const int len = (int)min((int64_t)t, sh.lbase[k + 1] - r0);       // (a row of the layout holds t values)
    if (len <= 0) return;                              // (the whole workgroup)
    for (int b = tid; b < G; b += AF_THREADS) { t_sum[b] = 0ull; t_lo[b] = ~0u; t_hi[b] = 0u; }
    __syncthreads();
    const double* __restrict__ row = vals + r0;
    uint32_t bad = 0;
#pragma unroll 1
    for (int base = 0; base < len; base += AF_THREADS) {             // (workgroup-uniform: the reduction below is the wave's)
        const int s = base + tid;
        uint32_t m = 0;
        int b = -1;
        if (s < len && af_micro(row[s], m, bad)) b = group[s];
        if ((unsigned)b >= (unsigned)G && b != -1) { ++bad; b = -1; }  // (the host has checked the labels: never)
        af_lds_add(b, m, lane, t_sum, t_lo, t_hi);
    }
    __syncthreads();
    PcAffinityEntry* const out = tab + (size_t)t * (size_t)G;
    for (int b = tid; b < G; b += AF_THREADS) {
        const uint32_t lo = t_lo[b];
        if (lo == ~0u) continue;                       // (no element of this row in group b: a counted element lowers lo to 10^6 or less)
        af_entry_add(out + b, t_sum[b], lo, t_hi[b]);
    }
    if (bad) (void)__hip_atomic_fetch_add(n_bad, (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// first j in [j0, j1) with member[j] >= x (j1: none); member ascends inside a group's run
__device__ __forceinline__ int af_lower(const int32_t* __restrict__ member, int j0, int j1, int x) {
    while (j0 < j1) { const int mid = j0 + (j1 - j0) / 2; if (member[mid] < x) j0 = mid + 1; else j1 = mid; }
    return j0;
}

// column pass: wave (blockIdx.y * AF_WAVES + wave) of source block blockIdx.x takes the groups [grange[u], grange[u + 1])
__global__ __launch_bounds__(AF_THREADS) void k_aff_cols(const double* __restrict__ vals, PcShard sh, int t0, int t1, const int32_t* __restrict__ member,
                                                        const int32_t* __restrict__ goff, const int32_t* __restrict__ grange, int n_ranges, int G,
                                                        PcAffinityEntry* __restrict__ tab, unsigned long long* __restrict__ /* n_bad: the row pass's */) {
    const int lane = threadIdx.x & 63;
    const int u = (int)blockIdx.y * AF_WAVES + (int)(threadIdx.x >> 6);
    if (u >= n_ranges) return;                         // (the whole wave)
    const int sb = (int)blockIdx.x * PC_AFFINITY_BLOCK, s = sb + lane;
    const int t_first = max(t0, sb + 1);               // the block's first target: above its first source, inside the slab
    if (t_first >= t1) return;                         // (the whole wave)
    const int a0 = grange[u], a1 = grange[u + 1];
    uint32_t bad = 0;                                  // (not reported: the row pass has seen every element of the slab and counted it once)
    for (int a = a0; a < a1; ++a) {
        const int g0 = goff[a], g1 = goff[a + 1];
        const int j0 = af_lower(member, g0, g1, t_first), j1 = af_lower(member, j0, g1, t1);
        if (j0 >= j1) continue;                        // (the whole wave: no member of a among the block's targets in this slab)
        unsigned long long sum = 0ull;
        uint32_t lo = ~0u, hi = 0u;
        for (int j = j0; j < j1; j += AF_UNROLL) {
            double v[AF_UNROLL];
            bool have[AF_UNROLL];
#pragma unroll
            for (int q = 0; q < AF_UNROLL; ++q) {      // (independent loads of 8 x block contiguous bytes each)
                have[q] = false; v[q] = 0.0;
                if (j + q < j1) {
                    const int t = member[j + q], k = t - t0;                 // (t0 <= t < t1 by the search: a row of the slab)
                    const int64_t r0 = sh.lbase[k];
                    have[q] = s < t && (int64_t)s < sh.lbase[k + 1] - r0;
                    if (have[q]) v[q] = vals[r0 + s];
                }
            }
#pragma unroll
            for (int q = 0; q < AF_UNROLL; ++q) {
                uint32_t m = 0;
                if (have[q] && af_micro(v[q], m, bad)) { sum += m; lo = m < lo ? m : lo; hi = m > hi ? m : hi; }
            }
        }
        if (lo != ~0u) af_entry_add(tab + (size_t)s * (size_t)G + a, sum, lo, hi);       // (s < some t < t1 <= N: a row of the table)
    }
}

// rows form, row pass: workgroup r takes row r of the rows slab -- query genome q = rows[r], table row r0 + r of the call (r0: the slab's
// first query row).  Every column s != q with a label is a pair of this row, whether s is a query genome or not; column q (the diagonal)
// and the columns of unlabelled genomes are not read.  The row is written whole by plain stores: a query's row lies in one slab.
// A refused value is left out and counted once per PAIR: a pair of two query genomes stands in two rows, and where both rows read it
// (both labelled) the row of the smaller counts it, as PcRowsDomain::live takes such a pair.
__global__ __launch_bounds__(AF_THREADS) void k_aff_qrows(const double* __restrict__ vals, PcRowsSlab dom, int r0, const int32_t* __restrict__ group, int G,
                                                         PcAffinityEntry* __restrict__ tab, unsigned long long* __restrict__ n_bad) {
    extern __shared__ unsigned long long af_table[];
    unsigned long long* const t_sum = af_table;
    uint32_t* const t_lo = (uint32_t*)(af_table + G);
    uint32_t* const t_hi = t_lo + G;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int n = dom.n, q = dom.rows[r];
    const bool q_labelled = group[q] >= 0;
    for (int b = tid; b < G; b += AF_THREADS) { t_sum[b] = 0ull; t_lo[b] = ~0u; t_hi[b] = 0u; }
    __syncthreads();
    const double* __restrict__ row = vals + (size_t)r * (size_t)n;
    uint32_t bad = 0;
#pragma unroll 1
    for (int base = 0; base < n; base += AF_THREADS) {                // (workgroup-uniform: the reduction is the wave's)
        const int s = base + tid;
        uint32_t m = 0;
        int b = -1;
        if (s < n && s != q) {
            const int bs = group[s];
            uint32_t refused = 0;
            if (bs >= 0) {
                if (af_micro(row[s], m, refused)) b = bs;
                else if (!(s < q && q_labelled && dom.is_query[s])) ++bad;      // (else row s reads the pair at column q, and counts it)
            }
        }
        if (b >= G) { ++bad; b = -1; }                 // (the host has checked the labels: never)
        af_lds_add(b, m, lane, t_sum, t_lo, t_hi);
    }
    __syncthreads();
    PcAffinityEntry* const out = tab + (size_t)(r0 + r) * (size_t)G;
    for (int b = tid; b < G; b += AF_THREADS) out[b] = PcAffinityEntry{t_sum[b], t_lo[b], t_hi[b]};
    if (bad) (void)__hip_atomic_fetch_add(n_bad, (unsigned long long)bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rows form, column pass (want_gain only): lane = column g, a wave 64 consecutive columns; what the slab's query genomes add to the own
// entry of an OLD labelled genome g -- the values of (g, x) over the query genomes x of the slab with group[x] == group[g].  A row's
// group is wave-uniform; its value is loaded only where some lane of the wave matches.  A lane keeps (sum, lo, hi) in registers and adds
// them into gain[g] once per slab: one writer per g and launch, slabs are successive launches on one stream.  Refused values are left
// out and not counted: the row pass has read the same elements.
__global__ __launch_bounds__(AF_THREADS) void k_aff_qcols(const double* __restrict__ vals, PcRowsSlab dom, const int32_t* __restrict__ group,
                                                         PcAffinityEntry* __restrict__ gain) {
    const int n = dom.n, g = (int)blockIdx.x * AF_THREADS + (int)threadIdx.x;
    const int mine = g < n && !dom.is_query[g] ? group[g] : -1;      // (-1: a query genome, an unlabelled one, or no column)
    if (!__any(mine >= 0)) return;                     // (the whole wave)
    unsigned long long sum = 0ull;
    uint32_t lo = ~0u, hi = 0u, bad = 0;               // (bad: not reported)
    for (int r = 0; r < dom.m; ++r) {
        const int gq = group[dom.rows[r]];             // (wave-uniform)
        const bool match = gq >= 0 && mine == gq;
        if (!__any(match)) continue;                   // (the whole wave)
        uint32_t m = 0;
        if (match && af_micro(vals[(size_t)r * (size_t)n + g], m, bad)) { sum += m; lo = m < lo ? m : lo; hi = m > hi ? m : hi; }
    }
    if (lo != ~0u) af_entry_add(gain + g, sum, lo, hi);
}

// staged: n_foreign tables of `bytes` each
__global__ __launch_bounds__(256) void k_aff_merge(PcAffinityEntry* __restrict__ tab, const char* __restrict__ staged, size_t bytes, int n_foreign, size_t n_entries) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_entries) return;
    PcAffinityEntry x = tab[idx];
    unsigned long long bad = 0ull;
    for (int f = 0; f < n_foreign; ++f) {
        const PcAffinityEntry* const o = (const PcAffinityEntry*)(staged + (size_t)f * bytes);
        const PcAffinityEntry y = o[idx];
        x.sum += y.sum; x.lo = y.lo < x.lo ? y.lo : x.lo; x.hi = y.hi > x.hi ? y.hi : x.hi;
        if (idx == 0) bad += *(const unsigned long long*)(o + n_entries);
    }
    tab[idx] = x;
    if (idx == 0) *(unsigned long long*)(tab + n_entries) += bad;
}

// is (sum_a, size_a, a) a smaller mean than (sum_b, size_b, b)?  a group index of INT32_MAX is none
__device__ __forceinline__ bool af_mean_less(unsigned long long sum_a, unsigned long long size_a, int a, unsigned long long sum_b, unsigned long long size_b, int b) {
    if (a == INT32_MAX) return false;
    if (b == INT32_MAX) return true;
    const unsigned long long l = sum_a * size_b, r = sum_b * size_a;
    return l < r || (l == r && a < b);
}

// The finish of ONE table row by one wave, shared by k_aff_finish (row g of the N x G table, own = group[g]) and k_aff_qfinish (row k of
// the n_rows x G table, own = the query genome's label or -1: it has no own group, its own entry is empty and every non-empty group is
// a candidate).  g: the row, and the place in the O(rows) arrays; N: their length (near_group is [3][N]).
__device__ __forceinline__ void af_finish_row(const PcAffinityEntry* __restrict__ row, int own, const int32_t* __restrict__ goff, int g, int N, int G, int invert,
                                              const PcAffinityOut& out, int lane) {
    // per lane, over its groups in ascending order: the best by each criterion (strictly better only: ties stay with the smaller index)
    unsigned long long m_sum = 0ull, m_size = 1ull;
    int m_idx = INT32_MAX;
    unsigned long long k_lo = ~0ull, k_hi = ~0ull;     // value << 32 | group
    for (int b = lane; b < G; b += 64) {
        const PcAffinityEntry e = row[b];
        const unsigned long long size = (unsigned long long)(goff[b + 1] - goff[b]), cnt = size - (b == own ? 1ull : 0ull);
        const bool empty = e.lo == ~0u;                // (cnt == 0, unless values were refused: then the call fails)
        unsigned long long sum = e.sum;
        uint32_t lo = e.lo, hi = e.hi;
        if (!empty && b != own) {
            if (af_mean_less(sum, cnt, b, m_sum, m_size, m_idx)) { m_sum = sum; m_size = cnt; m_idx = b; }
            const unsigned long long kl = ((unsigned long long)lo << 32) | (unsigned)b, kh = ((unsigned long long)hi << 32) | (unsigned)b;
            k_lo = kl < k_lo ? kl : k_lo; k_hi = kh < k_hi ? kh : k_hi;
        }
        if (invert && !empty) {                        // (lo <= hi <= 10^6 and sum <= cnt * 10^6: the passes admit nothing else)
            sum = cnt * 1000000ull - sum;
            const uint32_t l = 1000000u - hi;
            hi = 1000000u - lo; lo = l;
        }
        if (b == own) {
            out.own_sum[g] = (long long)sum;
            out.own_lo[g] = empty ? INT32_MAX : (int32_t)lo; out.own_hi[g] = empty ? -1 : (int32_t)hi;
        }
        if (out.tab_sum) {
            const size_t at = (size_t)g * (size_t)G + b;
            out.tab_sum[at] = (long long)sum;
            out.tab_lo[at] = empty ? INT32_MAX : (int32_t)lo; out.tab_hi[at] = empty ? -1 : (int32_t)hi;
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long os = __shfl_xor(m_sum, off), oz = __shfl_xor(m_size, off);
        const int oi = __shfl_xor(m_idx, off);
        if (af_mean_less(os, oz, oi, m_sum, m_size, m_idx)) { m_sum = os; m_size = oz; m_idx = oi; }
        const unsigned long long ol = __shfl_xor(k_lo, off), oh = __shfl_xor(k_hi, off);
        k_lo = ol < k_lo ? ol : k_lo; k_hi = oh < k_hi ? oh : k_hi;
    }
    if (lane != 0) return;
    const bool none = m_idx == INT32_MAX;              // (no other non-empty group: none by any criterion)
    const uint32_t v_lo = (uint32_t)(k_lo >> 32), v_hi = (uint32_t)(k_hi >> 32);
    out.near_group[g] = none ? -1 : m_idx;
    out.near_group[(size_t)N + g] = none ? -1 : (int32_t)(uint32_t)k_lo;
    out.near_group[2 * (size_t)N + g] = none ? -1 : (int32_t)(uint32_t)k_hi;
    out.near_sum[g] = none ? 0ll : (long long)(invert ? m_size * 1000000ull - m_sum : m_sum);
    out.near_lo[g] = none ? INT32_MAX : (int32_t)(invert ? 1000000u - v_lo : v_lo);
    out.near_hi[g] = none ? -1 : (int32_t)(invert ? 1000000u - v_hi : v_hi);
    if (own < 0) { out.own_sum[g] = 0ll; out.own_lo[g] = INT32_MAX; out.own_hi[g] = -1; }      // (the rows form's unlabelled query only)
}

// wave w of workgroup b takes genome b * AF_WAVES + w
__global__ __launch_bounds__(AF_THREADS) void k_aff_finish(const PcAffinityEntry* __restrict__ tab, const int32_t* __restrict__ group, const int32_t* __restrict__ goff,
                                                          int N, int G, int invert, PcAffinityOut out) {
    const int lane = threadIdx.x & 63;
    const int g = (int)blockIdx.x * AF_WAVES + (int)(threadIdx.x >> 6);
    if (g == 0 && threadIdx.x == 0) *out.bad = *(const unsigned long long*)(tab + (size_t)N * (size_t)G);
    if (g >= N) return;                                // (the whole wave)
    af_finish_row(tab + (size_t)g * (size_t)G, group[g], goff, g, N, G, invert, out, lane);
}

// rows form.  Workgroups [0, ceil(n_rows / AF_WAVES)): wave w of workgroup b takes query row k = b * AF_WAVES + w -- row k of the table,
// own group that of genome rows[k].  goff counts the LABELLED genomes of each group, queries included.  The workgroups behind them
// (want_gain only: gout.sum != NULL) take AF_THREADS genomes each, a thread a genome: gain[g] converted (an empty entry as 0 / INT32_MAX /
// -1) and, for a similarity statement, complemented over its count, qcount[group[g]] -- the query genomes of g's group (from the host).
// tab: PcAffinityEntry[n_rows][G] | gain[N] | the violation count.
__global__ __launch_bounds__(AF_THREADS) void k_aff_qfinish(const PcAffinityEntry* __restrict__ tab, const int32_t* __restrict__ rows, const int32_t* __restrict__ group,
                                                           const int32_t* __restrict__ goff, const int32_t* __restrict__ qcount, int n_rows, int N, int G,
                                                           int invert, PcAffinityOut out, PcAffinityGainOut gout) {
    const int row_blocks = (n_rows + AF_WAVES - 1) / AF_WAVES;
    const PcAffinityEntry* const gain = tab + (size_t)n_rows * (size_t)G;
    if ((int)blockIdx.x >= row_blocks) {
        const int g = ((int)blockIdx.x - row_blocks) * AF_THREADS + (int)threadIdx.x;
        if (g >= N) return;
        const PcAffinityEntry e = gain[g];
        const bool empty = e.lo == ~0u;                // (else g is an old labelled genome: the column pass adds nowhere else)
        unsigned long long sum = e.sum;
        uint32_t lo = e.lo, hi = e.hi;
        if (invert && !empty) {
            sum = (unsigned long long)qcount[group[g]] * 1000000ull - sum;
            const uint32_t l = 1000000u - hi;
            hi = 1000000u - lo; lo = l;
        }
        gout.sum[g] = (long long)sum; gout.lo[g] = empty ? INT32_MAX : (int32_t)lo; gout.hi[g] = empty ? -1 : (int32_t)hi;
        return;
    }
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * AF_WAVES + (int)(threadIdx.x >> 6);
    if (k == 0 && threadIdx.x == 0) *out.bad = *(const unsigned long long*)(gain + N);
    if (k >= n_rows) return;                           // (the whole wave)
    af_finish_row(tab + (size_t)k * (size_t)G, group[rows[k]], goff, k, n_rows, G, invert, out, lane);
}

static bool affinity_shape_ok(int N, int G, const char* what) {
    if (N >= 1 && G >= 1 && G <= PC_BETWEEN_MAX_GROUPS) return true;
    pc_set_error("%s: %d genomes in %d groups (1 .. PC_BETWEEN_MAX_GROUPS = %d)", what, N, G, PC_BETWEEN_MAX_GROUPS);
    return false;
}
static unsigned long long* affinity_bad(void* tab, int N, int G) { return (unsigned long long*)((PcAffinityEntry*)tab + (size_t)N * (size_t)G); }
static int affinity_grid(size_t n_entries, const char* what, dim3& grid) {
    const size_t blocks = (n_entries + 255) / 256;
    if (blocks > 0x7fffffffull) { pc_set_error("%s: %zu entries", what, n_entries); return PC_ERR_LIMIT; }
    grid = dim3((unsigned)blocks);
    return PC_OK;
}

int pc_launch_affinity_init(void* tab, int N, int G, hipStream_t st) {
    if (!affinity_shape_ok(N, G, "k_aff_init")) return PC_ERR_ARG;
    dim3 grid;
    int rc = affinity_grid((size_t)N * (size_t)G, "k_aff_init", grid);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_aff_init, grid, dim3(256), 0, st, (PcAffinityEntry*)tab, (size_t)N * (size_t)G);
    return pc_launch_check("k_aff_init");
}

// the slab's targets are [t0, t0 + sh.nown), row k of the shard target t0 + k
int pc_launch_affinity_rows(const double* vals, int64_t Lp, const PcShard& sh, int t0, int N, const int32_t* group, int G, void* tab, hipStream_t st) {
    if (Lp <= 0 || sh.nown <= 0) return PC_OK;
    if (!affinity_shape_ok(N, G, "k_aff_rows")) return PC_ERR_ARG;
    if (t0 < 0 || (int64_t)t0 + sh.nown > N) { pc_set_error("k_aff_rows: targets [%d, %lld) of %d", t0, (long long)t0 + sh.nown, N); return PC_ERR_ARG; }
    hipLaunchKernelGGL(k_aff_rows, dim3((unsigned)sh.nown), dim3(AF_THREADS), (size_t)G * 16, st, vals, sh, t0, group, G, (PcAffinityEntry*)tab,
                       affinity_bad(tab, N, G));
    return pc_launch_check("k_aff_rows");
}

int pc_launch_affinity_cols(const double* vals, int64_t Lp, const PcShard& sh, int t0, int N, const int32_t* member, const int32_t* goff,
                            const int32_t* grange, int n_ranges, int G, void* tab, hipStream_t st) {
    if (Lp <= 0 || sh.nown <= 0) return PC_OK;
    if (!affinity_shape_ok(N, G, "k_aff_cols")) return PC_ERR_ARG;
    const int64_t t1 = (int64_t)t0 + sh.nown;
    if (t0 < 0 || t1 > N || n_ranges < 1 || n_ranges > G) { pc_set_error("k_aff_cols: targets [%d, %lld) of %d, %d group ranges", t0, (long long)t1, N, n_ranges); return PC_ERR_ARG; }
    if (t1 < 2) return PC_OK;                          // (target 0 alone has no source)
    const dim3 grid((unsigned)((t1 - 1 + PC_AFFINITY_BLOCK - 1) / PC_AFFINITY_BLOCK), (unsigned)((n_ranges + AF_WAVES - 1) / AF_WAVES));
    if (grid.y > 65535u) { pc_set_error("k_aff_cols: %d group ranges", n_ranges); return PC_ERR_ARG; }
    hipLaunchKernelGGL(k_aff_cols, grid, dim3(AF_THREADS), 0, st, vals, sh, t0, (int)t1, member, goff, grange, n_ranges, G, (PcAffinityEntry*)tab,
                       affinity_bad(tab, N, G));
    return pc_launch_check("k_aff_cols");
}

int pc_launch_affinity_merge(void* tab, const void* staged, int n_foreign, int N, int G, hipStream_t st) {
    if (n_foreign <= 0) return PC_OK;
    if (!affinity_shape_ok(N, G, "k_aff_merge")) return PC_ERR_ARG;
    dim3 grid;
    int rc = affinity_grid((size_t)N * (size_t)G, "k_aff_merge", grid);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_aff_merge, grid, dim3(256), 0, st, (PcAffinityEntry*)tab, (const char*)staged, pc_affinity_table_bytes(N, G), n_foreign,
                       (size_t)N * (size_t)G);
    return pc_launch_check("k_aff_merge");
}

int pc_launch_affinity_finish(const void* tab, const int32_t* group, const int32_t* goff, int N, int G, int invert, void* out, int want_table, hipStream_t st) {
    if (!affinity_shape_ok(N, G, "k_aff_finish")) return PC_ERR_ARG;
    hipLaunchKernelGGL(k_aff_finish, dim3((unsigned)((N + AF_WAVES - 1) / AF_WAVES)), dim3(AF_THREADS), 0, st, (const PcAffinityEntry*)tab, group, goff, N, G,
                       invert ? 1 : 0, pc_affinity_out_view(out, N, G, want_table));
    return pc_launch_check("k_aff_finish");
}

// ---- the rows form ----
static bool affinity_rows_shape_ok(int n_rows, int N, int G, const char* what) {
    if (N >= 1 && n_rows >= 1 && n_rows <= N && G >= 1 && G <= PC_BETWEEN_MAX_GROUPS) return true;
    pc_set_error("%s: %d query rows of %d genomes in %d groups (1 .. PC_BETWEEN_MAX_GROUPS = %d)", what, n_rows, N, G, PC_BETWEEN_MAX_GROUPS);
    return false;
}

int pc_launch_affinity_rows_init(void* state, int n_rows, int N, int G, hipStream_t st) {
    if (!affinity_rows_shape_ok(n_rows, N, G, "k_aff_init")) return PC_ERR_ARG;
    const size_t n_entries = pc_affinity_rows_entries(n_rows, N, G);
    dim3 grid;
    int rc = affinity_grid(n_entries, "k_aff_init", grid);
    if (rc != PC_OK) return rc;
    hipLaunchKernelGGL(k_aff_init, grid, dim3(256), 0, st, (PcAffinityEntry*)state, n_entries);
    return pc_launch_check("k_aff_init");
}

int pc_launch_affinity_rows_slab(const double* vals, int64_t Lp, const PcRowsSlab& dom, int r0, int n_rows, const int32_t* group, int G, void* state,
                                 int want_gain, hipEvent_t between, hipStream_t st) {
    const int N = dom.n, m = dom.m;
    if (!affinity_rows_shape_ok(n_rows, N, G, "k_aff_qrows")) return PC_ERR_ARG;
    if (m < 1 || r0 < 0 || (int64_t)r0 + m > n_rows || Lp != (int64_t)m * N) {
        pc_set_error("k_aff_qrows: a slab of %d x %d at query row %d of %d is not %lld values", m, N, r0, n_rows, (long long)Lp);
        return PC_ERR_ARG;
    }
    PcAffinityEntry* const tab = (PcAffinityEntry*)state;
    PcAffinityEntry* const gain = tab + (size_t)n_rows * (size_t)G;
    hipLaunchKernelGGL(k_aff_qrows, dim3((unsigned)m), dim3(AF_THREADS), (size_t)G * 16, st, vals, dom, r0, group, G, tab, (unsigned long long*)(gain + N));
    int rc = pc_launch_check("k_aff_qrows");
    if (rc != PC_OK) return rc;
    if (between) PC_HIP(hipEventRecord(between, st));
    if (!want_gain) return PC_OK;
    hipLaunchKernelGGL(k_aff_qcols, dim3((unsigned)((N + AF_THREADS - 1) / AF_THREADS)), dim3(AF_THREADS), 0, st, vals, dom, group, gain);
    return pc_launch_check("k_aff_qcols");
}

int pc_launch_affinity_rows_finish(const void* state, const int32_t* rows, const int32_t* group, const int32_t* goff, const int32_t* qcount, int n_rows, int N,
                                   int G, int invert, void* out, int want_table, int want_gain, hipStream_t st) {
    if (!affinity_rows_shape_ok(n_rows, N, G, "k_aff_qfinish")) return PC_ERR_ARG;
    const unsigned blocks = (unsigned)((n_rows + AF_WAVES - 1) / AF_WAVES) + (want_gain ? (unsigned)((N + AF_THREADS - 1) / AF_THREADS) : 0u);
    hipLaunchKernelGGL(k_aff_qfinish, dim3(blocks), dim3(AF_THREADS), 0, st, (const PcAffinityEntry*)state, rows, group, goff, qcount, n_rows, N, G,
                       invert ? 1 : 0, pc_affinity_out_view(out, n_rows, G, want_table), pc_affinity_gain_view(out, n_rows, N, G, want_table, want_gain));
    return pc_launch_check("k_aff_qfinish");
}
