// pc_tree.hip -- the kernels of pc_fill_tree: the single-linkage dendrogram of the collection as the minimum spanning tree of the
// complete graph over the genomes, under ONE strict total order on the pairs -- the better value first, then the smaller target t,
// then the smaller source s -- which is one word per pair: key = micro << 44 | t << 22 | s (pc_common.h; micro = the value in
// millionths, on a similarity fill 10^6 minus it).  An unsigned 64-bit minimum is the minimum of the order; PC_TREE_NONE (~0) is no key.
// The order is strict, so the tree is unique: it is the one Kruskal's algorithm accepts, whatever the slab cut, the number of devices
// or the outcome of any race.  MST(A + B) = MST(MST(A) + B): a forest of at most N - 1 keys ("list") stays on the device across the
// slabs, and every slab goes through one PASS of Boruvka rounds over that list and the slab, from scratch, into a second list; then the
// two lists swap.  MST(A + B) = MST(MST(A) + MST(B)): several devices' lists merge on the root by a pass over lists alone.
//   k_tree_reset        comp[g] = g, best[g] = none, the new list emptied (it takes the old list's counters over), live[0] = 1
//   one round r, four launches, each returning at once when live[r] == 0 (the round before it joined nothing):
//   k_tree_scan_slab    ONE body, pc_tree_scan_body, under two kernels: k_tree_scan_slab over a triangular slab (PcTriDomain) and
//                       k_tree_scan_rows over a rows slab (PcRowsDomain; pc_fill_rows_tree: the LIVE elements only).  It streams the
//                       slab as every slab pass does (pc_slab_pass.h: flat f64[Lp], chunks of 4,096 elements, 16-byte loads, the odd
//                       last element alone, nothing read beyond Lp) and takes an element's two genomes from the domain; a pair whose ends
//                       lie in different components lowers best[comp[s]] and best[comp[t]] to its key
//   k_tree_scan_list    the same over a list of keys, s and t decoded from the key (the resident forest; on the root of a
//                       several-device call the other devices' forests)
//   k_tree_hook         a root c with an edge: d = the component of the edge's other end; next[c] = d, unless d chose the same edge
//                       and c < d: then c stays a root.  The key is appended to the new list, once per edge; live[r + 1] = 1
//   k_tree_flatten      comp[g] = the root the next-chain above comp[g] ends in; best[g] = none
// Invariants, between rounds:
//   J1  comp[g] is a root (comp[comp[g]] == comp[g]) and g is connected to it by edges of the new list: comp[] names the components
//       of the graph the new list spans.
//   J2  every key of the new list is an edge of THE tree of (old list + slab): a round appends, per component C, the smallest edge
//       leaving C, and by the cut property under a strict order that edge belongs to the unique minimum spanning tree.
//   J3  best[] is none everywhere (reset, flatten).
// The pick graph of a round (an arrow from every root with an edge to the component its smallest outgoing edge leads to) is a forest
// with exactly one doubly-chosen edge per tree: follow the arrows from any root -- the keys chosen along the way never increase (each
// root chose its smallest edge, and the edge it was reached by is one of its edges), and keys of different pairs differ, so the walk
// can only close on a cycle of two roots that chose the SAME edge; every root has one arrow, so each connected piece holds exactly
// one such cycle.  k_tree_hook breaks it by index (the smaller of the two stays the root, and appends the edge; the larger does
// neither), which leaves a rooted tree per piece: the chains k_tree_flatten follows end, and every chosen edge is appended once.  An
// edge joins two different components of a forest, so no cycle forms in the list and it never holds more than N - 1 keys.
// Rounds: every component that has an outgoing edge is joined with at least one other, so their number at least halves per round:
// ceil(log2 N) rounds leave none.  They are enqueued blind; nothing is read back.  A pass ends with the new list = the tree of
// (old list + slab): by J2 its keys are tree edges, and when no component has an outgoing edge left it spans what the input spans.
// What is atomic and why: inside k_tree_scan_* best[] is touched ONLY by relaxed agent-scope atomics (an atomic load, then an atomic
// unsigned minimum): the XCDs' L2s are not coherent with each other, and a minimum must not be lost.  best[] only decreases inside a
// launch, so a stale read lets a needless atomic through and never drops a smaller key.  Scattered atomics are the expensive part,
// so no lane issues one it can avoid: a key that does not beat the word it read is skipped, and the lanes of a wave that share a
// component on the side the domain names (a wave reads 128 consecutive elements: mostly one target genome of a triangular slab, mostly
// one row of a rows slab, i.e. the QUERY genome, whether it is the pair's source or its target) reduce their keys in the wave first --
// at most one atomic per component and wave on that side; the other side is lowered at once.  comp[] is written by k_tree_flatten /
// k_tree_reset only, launches of their own: plain loads elsewhere.  k_tree_hook reads best[] after the scans' launches ended (plain
// loads) and takes list slots with one returning atomic add per wave on the list's count; live[r + 1] is set by an atomic store of the
// same value from every wave that appended.  k_tree_flatten reads next[] (written by the hook launch) and writes its own words only.
// Progress: no workgroup ever waits for another; no flag is spun on; nothing sleeps.  The loops are the triangular domain's forward
// walk over lbase (bounded by the chunk's rows), the wave's reduction (one turn per distinct shared component among 64 lanes) and the
// chain walk (bounded by the chain, and by n).
// The scan checks what the key relies on -- k = rint(v * 1e6) lies in [0, 10^6] and pc_div_million(k) == v bit for bit -- and counts
// what fails it in the list's violation word: the host answers a non-zero count with PC_ERR_DATA.
#include "pc_slab_pass.h"

typedef unsigned long long tree_key_t;

__device__ __forceinline__ tree_key_t pc_tree_read(const tree_key_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// best[c] = min(best[c], key), the atomic skipped when the word already holds a key at least as good
__device__ __forceinline__ void pc_tree_lower(tree_key_t* best, int c, tree_key_t key) {
    if (key < pc_tree_read(best + c)) __hip_atomic_fetch_min(best + c, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The same for a whole wave (every lane calls; c < 0: nothing to lower): lanes that share c reduce their keys first, one atomic per c.
__device__ __forceinline__ void pc_tree_lower_shared(tree_key_t* best, int c, tree_key_t key, int lane) {
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {                                     // (wave-uniform: one turn per distinct c)
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(c, leader);
        const bool mine = c == lc;
        tree_key_t m = mine ? key : PC_TREE_NONE;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const tree_key_t o = __shfl_xor(m, off);
            m = o < m ? o : m;
        }
        if (lane == leader) pc_tree_lower(best, lc, m);
        todo &= ~__ballot(mine);
    }
}

// the key of pair (s, t) with value v, or none (and one violation) when v is not a millionth in [0, 1]
// (an f64 compare: of bits for everything but the two zeros -- -0.0 is the millionth 0, and pc_div_million(-0.0) is +0.0)
template <int DIST> __device__ __forceinline__ tree_key_t pc_tree_pair_key(double v, int s, int t, uint32_t& bad) {
    const double k = __builtin_rint(v * 1.0e6);
    if (!(k >= 0.0 && k <= 1.0e6) || pc_div_million(k) != v) { ++bad; return PC_TREE_NONE; }
    const int ki = (int)k;
    return pc_tree_key_of(DIST ? ki : PC_TREE_MICRO_MAX - ki, s, t);
}

// One element, the pair of genome a -- on the side the wave's lanes mostly share -- and genome b: its key, b's side lowered at once,
// and a's component when the key may still beat best[] there (else -1).  comp: [n], a, b < n.
template <int DIST, class Dom> __device__ __forceinline__ void pc_tree_element(double v, int a, int b, const int32_t* __restrict__ comp, tree_key_t* best,
                                                                               tree_key_t& key, int& shared_out, uint32_t& bad) {
    key = PC_TREE_NONE; shared_out = -1;
    const int cb = comp[b], ca = comp[a];
    if (ca == cb) return;
    int s, t;
    Dom::sorted(a, b, s, t);
    key = pc_tree_pair_key<DIST>(v, s, t, bad);
    if (key == PC_TREE_NONE) return;
    pc_tree_lower(best, cb, key);
    if (key < pc_tree_read(best + ca)) shared_out = ca;
}

__global__ __launch_bounds__(256) void k_tree_reset(int32_t* __restrict__ comp, tree_key_t* __restrict__ best, uint32_t* __restrict__ live, int rounds,
                                                    const tree_key_t* in, tree_key_t* out, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < n) { comp[g] = g; best[g] = PC_TREE_NONE; }
    if (g == 0) {
        out[n - 1] = 0ull;
        out[n] = in ? in[n] : 0ull;
        out[n + 1] = in ? in[n + 1] : 0ull;
        live[0] = 1u;
        for (int r = 1; r <= rounds; ++r) live[r] = 0u;
    }
}

__global__ void k_tree_take_counts(tree_key_t* out, const tree_key_t* __restrict__ lists, int n_foreign, int n) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int f = 0; f < n_foreign; ++f) {
        const tree_key_t* list = lists + (size_t)f * ((size_t)n + PC_TREE_TAIL);
        out[n] += list[n];
        out[n + 1] += list[n + 1];
    }
}

// (no barrier but the one that hands the chunk's place on: either domain is located ahead of the loads)
template <int DIST, class Dom>
__device__ __forceinline__ void pc_tree_scan_body(const double* __restrict__ vals, int64_t Lp, const Dom dom, const int32_t* __restrict__ comp,
                                                  tree_key_t* best, tree_key_t* out, int n, const uint32_t* __restrict__ live) {
    if (*live == 0u) return;                           // (the whole grid)
    __shared__ typename Dom::Origin origin;
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * SLAB_CHUNK + (int64_t)threadIdx.x * 2;
    pc_slab_locate(dom, origin);
    __syncthreads();
    typename Dom::Cursor at = dom.start(origin);
    uint32_t bad = 0;
#pragma unroll 1
    for (int j = 0; j < SLAB_ITERS; ++j) {             // (every lane takes every turn: the reductions below are the wave's)
        double a, b;
        const int64_t i = base + (int64_t)j * SLAB_STRIDE;
        const int have = pc_slab_load(vals, i, Lp, a, b);
        tree_key_t key_a = PC_TREE_NONE, key_b = PC_TREE_NONE;
        int c_a = -1, c_b = -1, ga, gb;
        if (have > 0 && dom.live(at, i)) { dom.pair(at, i, ga, gb); pc_tree_element<DIST, Dom>(a, ga, gb, comp, best, key_a, c_a, bad); }
        if (have > 1 && dom.live(at, i + 1)) { dom.pair(at, i + 1, ga, gb); pc_tree_element<DIST, Dom>(b, ga, gb, comp, best, key_b, c_b, bad); }
        if (c_b >= 0 && c_b == c_a) { key_a = key_b < key_a ? key_b : key_a; c_b = -1; }
        else if (c_b >= 0 && c_a < 0) { key_a = key_b; c_a = c_b; c_b = -1; }
        pc_tree_lower_shared(best, c_a, key_a, lane);
        if (__any(c_b >= 0)) pc_tree_lower_shared(best, c_b, key_b, lane);        // (a lane whose two elements lie in two rows)
        dom.step(at);
    }
    if (bad) atomicAdd(out + n, (unsigned long long)bad);
}

template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_tree_scan_slab(const double* __restrict__ vals, int64_t Lp, PcShard sh, const int32_t* __restrict__ comp,
                                                                 tree_key_t* best, tree_key_t* out, int n, const uint32_t* __restrict__ live) {
    pc_tree_scan_body<DIST>(vals, Lp, PcTriDomain{sh}, comp, best, out, n, live);
}
template <int DIST>
__global__ __launch_bounds__(SLAB_THREADS) void k_tree_scan_rows(const double* __restrict__ vals, int64_t Lp, PcRowsSlab dom, const int32_t* __restrict__ comp,
                                                                 tree_key_t* best, tree_key_t* out, int n, const uint32_t* __restrict__ live) {
    pc_tree_scan_body<DIST>(vals, Lp, PcRowsDomain{dom}, comp, best, out, n, live);
}

// list: [n + PC_TREE_TAIL], list[n - 1] keys in it
__global__ __launch_bounds__(256) void k_tree_scan_list(const tree_key_t* __restrict__ list, const int32_t* __restrict__ comp, tree_key_t* best, int n,
                                                        const uint32_t* __restrict__ live) {
    if (*live == 0u) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n - 1 || (tree_key_t)i >= list[n - 1]) return;
    const tree_key_t key = list[i];
    const int s = pc_tree_key_s(key), t = pc_tree_key_t(key);
    if (s >= n || t >= n) return;                      // (no key of this collection; the host refuses such a list when it decodes it)
    const int cs = comp[s], ct = comp[t];
    if (cs == ct) return;
    pc_tree_lower(best, cs, key);
    pc_tree_lower(best, ct, key);
}

// live: live[0] this round's word, live[1] the next round's
__global__ __launch_bounds__(256) void k_tree_hook(const int32_t* __restrict__ comp, int32_t* __restrict__ next, const tree_key_t* __restrict__ best,
                                                   tree_key_t* out, int n, uint32_t* live) {
    if (live[0] == 0u) return;
    const int c = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    bool emit = false;
    tree_key_t b = PC_TREE_NONE;
    if (c < n && comp[c] == c) {
        int d = c;
        b = best[c];
        if (b != PC_TREE_NONE) {
            const int cs = comp[pc_tree_key_s(b)], ct = comp[pc_tree_key_t(b)];
            d = cs == c ? ct : cs;
            const bool both = best[d] == b;            // the same edge, chosen from both sides
            if (both && c < d) d = c;                  // ... the smaller index stays a root, and appends it
            emit = !both || d == c;
        }
        next[c] = d;
    }
    const unsigned long long m = __ballot(emit);
    if (m == 0ull) return;                             // (the whole wave)
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long at = 0ull;
    if (lane == leader) {
        at = atomicAdd(out + (n - 1), (unsigned long long)__popcll(m));
        __hip_atomic_store(live + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    at = __shfl(at, leader);
    if (emit) {
        const unsigned long long p = at + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (p < (unsigned long long)(n - 1)) out[p] = b;           // (a forest of n nodes has at most n - 1 edges: never beyond the keys)
    }
}

__global__ __launch_bounds__(256) void k_tree_flatten(int32_t* comp, const int32_t* __restrict__ next, tree_key_t* __restrict__ best, tree_key_t* out,
                                                      int n, const uint32_t* __restrict__ live) {
    if (*live == 0u) return;
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    int r = comp[g], p = next[r];
    for (int step = 0; p != r && step < n; ++step) { r = p; p = next[r]; }
    comp[g] = r;
    best[g] = PC_TREE_NONE;
    if (g == 0) out[n + 1] += 1ull;                    // a round that did work
}

static dim3 tree_grid(int n) { return dim3((unsigned)((std::max(n, 1) + 255) / 256)); }

int pc_tree_round_count(int n) {
    int rounds = 1;
    while ((1 << rounds) < n && rounds < 30) ++rounds;
    return rounds;
}

// comp, best: [n]; live: [rounds + 1]; in (or NULL), out: lists of n + PC_TREE_TAIL words; n >= 2
int pc_launch_tree_reset(int32_t* comp, unsigned long long* best, uint32_t* live, int rounds, const unsigned long long* in, unsigned long long* out,
                         int n, hipStream_t st) {
    if (n < 2) return PC_OK;
    hipLaunchKernelGGL(k_tree_reset, tree_grid(n), dim3(256), 0, st, comp, best, live, rounds, in, out, n);
    return pc_launch_check("k_tree_reset");
}

int pc_launch_tree_take_counts(unsigned long long* out, const unsigned long long* lists, int n_foreign, int n, hipStream_t st) {
    if (n_foreign <= 0 || n < 2) return PC_OK;
    hipLaunchKernelGGL(k_tree_take_counts, dim3(1), dim3(64), 0, st, out, lists, n_foreign, n);
    return pc_launch_check("k_tree_take_counts");
}

// dom: the slab's shard or rows domain, its tables on the device, every genome of its pairs below n; comp, best: [n]; out: the list
// that takes the violations
int pc_launch_tree_scan_slab(const double* vals, int64_t Lp, int as_distance, PcSlabDomain dom, const int32_t* comp, unsigned long long* best,
                             unsigned long long* out, int n, const uint32_t* live, int r, hipStream_t st) {
    if (Lp <= 0 || n < 2) return PC_OK;
    const char* const what = dom.is_rows ? "k_tree_scan_rows" : "k_tree_scan_slab";
    if (dom.is_rows && (dom.rows.n != n || dom.rows.m <= 0 || Lp != (int64_t)dom.rows.m * dom.rows.n)) { pc_set_error("%s: a rows slab of %d x %d is not %lld values of %d genomes", what, dom.rows.m, dom.rows.n, (long long)Lp, n); return PC_ERR_ARG; }
    const int rc = pc_slab_domain_check(dom, Lp, what);
    if (rc != PC_OK) return rc;
    const dim3 grid((unsigned)pc_edge_chunks(Lp)), block(SLAB_THREADS);
    pc_dispatch<0, 1>(as_distance ? 1 : 0, [&](auto dist) {
        constexpr int DIST = decltype(dist)::value;
        if (dom.is_rows) hipLaunchKernelGGL((k_tree_scan_rows<DIST>), grid, block, 0, st, vals, Lp, dom.rows, comp, best, out, n, live + r);
        else hipLaunchKernelGGL((k_tree_scan_slab<DIST>), grid, block, 0, st, vals, Lp, dom.shard, comp, best, out, n, live + r);
    });
    return pc_launch_check(what);
}

int pc_launch_tree_scan_list(const unsigned long long* list, const int32_t* comp, unsigned long long* best, int n, const uint32_t* live, int r,
                             hipStream_t st) {
    if (n < 2) return PC_OK;
    hipLaunchKernelGGL(k_tree_scan_list, tree_grid(n - 1), dim3(256), 0, st, list, comp, best, n, live + r);
    return pc_launch_check("k_tree_scan_list");
}

int pc_launch_tree_hook(const int32_t* comp, int32_t* next, const unsigned long long* best, unsigned long long* out, int n, uint32_t* live, int r,
                        hipStream_t st) {
    if (n < 2) return PC_OK;
    hipLaunchKernelGGL(k_tree_hook, tree_grid(n), dim3(256), 0, st, comp, next, best, out, n, live + r);
    return pc_launch_check("k_tree_hook");
}

int pc_launch_tree_flatten(int32_t* comp, const int32_t* next, unsigned long long* best, unsigned long long* out, int n, const uint32_t* live, int r,
                           hipStream_t st) {
    if (n < 2) return PC_OK;
    hipLaunchKernelGGL(k_tree_flatten, tree_grid(n), dim3(256), 0, st, comp, next, best, out, n, live + r);
    return pc_launch_check("k_tree_flatten");
}
