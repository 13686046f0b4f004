// pc_walk.hip -- the shared-pham walker over its four pair domains: k_walk (whole fills: pocp / af, alignment counting and planning,
// the best-match reduce of aai / peq), k_walk_rows (rows fills: the same and gcs / jc), k_walk_groups (groups fills: as the rows
// walker, over the within-group pairs of a family of groups) and k_walk_pairs (pair-list fills: as the rows walker, over a flat list
// of oriented pairs).  One core -- the visit of a shared pham, the visits of a bitmap word, the value epilogue, the COUNT totals --
// serves all four kernels, so each rule of the reference is stated once.  k_walk and k_walk_pairs also run in a JOINT mode: PEQ's walk
// over the alignment results, with up to six metrics of the pair out of its visits (pc_walk_joint_values: one store per metric asked for).
//
// Reference semantics restated here (metrics.py of the reference unless named):
//   metrics.py:83-115, 118-157   pocp / af: sums over shared phams of gene counts / lengths     (pc_visit, pc_walk_value)
//   metrics.py:203-227           aai: anchor rule, best match (ties -> last), weighted mean      (pc_visit, pc_walk_value)
//   metrics.py:247-253           peq = round(af, 6) * round(aai, 6), then round(., 6)            (pc_walk_value)
//   matrix.py:169-213, 467-486   the rows domain: source = min, target = max, the diagonal      (k_walk_rows)
//   matrix.py:155-167, 479-486   the groups domain: a sub-matrix's pairs, source = the smaller index (k_walk_groups)
//   metrics.py:26-253            the pairs domain: METRICS[metric](source, target) as called        (k_walk_pairs)
#include "pc_pairs.h"

#define WCH 32         // bitmap words staged per chunk (17 KB of LDS per workgroup: nine workgroups per CU hide the staging latency)

// The walker visits the shared phams of each pair in ascending pham id; entry index of pham p in genome g = rankpre[g][p>>6] +
// popcount(B[g][p>>6] below bit p).
struct PcPairAcc {
    uint32_t k;            // running alignment slot (ENUM / AAI / PEQ), alignment count (COUNT) or |S n T| (GCS / JC)
    int64_t cons;          // conserved gene count (POCP) or conserved length (AF / PEQ)
    double num;            // sum of best_ident/len * len   (statistics.py:22 numerator)
    int64_t den;           // sum of best lengths (COUNT: the pair's DP cells)
    int any;               // shared set non-empty
    __device__ __forceinline__ void reset() { k = 0; cons = 0; num = 0.0; den = 0; any = 0; }
};
// JOINT walks as PEQ does (k the slot cursor, cons the conserved length) and keeps beside it what the other metrics read of the same visits
struct PcJointAcc : PcPairAcc {
    uint32_t shared;       // |S n T|: the visits (GCS / JC)
    int64_t genes;         // conserved gene count (POCP)
    __device__ __forceinline__ void reset() { PcPairAcc::reset(); shared = 0; genes = 0; }
};
// What a mode accumulates in and is launched with: JOINT's own, every other mode's as before.  (Specialisations, not a condition on
// MODE: a kernel's signature names PcWalkModeTypes<MODE> and nothing else, so its mangled name does not depend on the modes' enum.)
template <int MODE> struct PcWalkModeTypes { using Acc = PcPairAcc; using Args = PcWalkArgs; };
template <> struct PcWalkModeTypes<PCW_JOINT> { using Acc = PcJointAcc; using Args = PcJointArgs; };
template <int MODE> using PcAccOf = typename PcWalkModeTypes<MODE>::Acc;
template <int MODE> using PcArgsOf = typename PcWalkModeTypes<MODE>::Args;
// the modes that walk a pair's alignment slots from a.off on
__host__ __device__ constexpr bool pc_walks_slots(int mode) { return mode == PCW_ENUM || mode == PCW_AAI || mode == PCW_PEQ || mode == PCW_JOINT; }

template <int MODE>
__device__ __forceinline__ void pc_visit(const PcDev& d, const PcWalkArgs& a, PcAccOf<MODE>& p, uint32_t es, uint32_t et,
                                         unsigned long long& cells, unsigned long long& rbytes) {
    p.any = 1;
    if constexpr (MODE == PCW_JOINT) { ++p.shared; p.genes += d.ent_cnt[es] + d.ent_cnt[et]; }   // GCS / JC's count, POCP's sum (metrics.py:102-103)
    if (MODE == PCW_POCP) { p.cons += d.ent_cnt[es] + d.ent_cnt[et]; return; }          // metrics.py:102-103
    if (MODE == PCW_AF) { p.cons += d.ent_len[es] + d.ent_len[et]; return; }            // metrics.py:135-147
    const int cs = d.ent_cnt[es], ct = d.ent_cnt[et];
    // anchor = the genome with fewer genes in the pham; tie -> source (metrics.py:208-209)
    const bool swap = cs > ct;
    const uint32_t ea = swap ? et : es, eb = swap ? es : et;
    const int ca = swap ? ct : cs, cb = swap ? cs : ct;
    const int a0 = d.ent_gene[ea], b0 = d.ent_gene[eb];
    if (MODE == PCW_COUNT) {
        p.k += (uint32_t)(ca * cb);
        const unsigned long long la = (unsigned long long)d.ent_len[ea], lb = (unsigned long long)d.ent_len[eb];
        cells += la * lb;
        p.den += (int64_t)(la * lb);                                                     // per pair, for the cost-balanced deal
        rbytes += la * cb + lb * ca;
    } else if (MODE == PCW_ENUM) {                                                        // sort key per alignment slot (pc_plan.hip)
        for (int ia = 0; ia < ca; ++ia) {
            const unsigned long long qa = d.gene_q[a0 + ia];
            for (int ib = 0; ib < cb; ++ib) {
                const uint32_t k = p.k++;
                a.key[k] = ((unsigned long long)d.gene_q[b0 + ib] << d.ubits) | qa;
                a.val[k] = k;
            }
        }
    } else {                                                                              // AAI / PEQ / JOINT
        if (MODE == PCW_PEQ || MODE == PCW_JOINT) p.cons += d.ent_len[es] + d.ent_len[et];
        for (int ia = 0; ia < ca; ++ia) {
            double best = -1.0; uint32_t best_len = 0;
            for (int ib = 0; ib < cb; ++ib) {
                const uint2 r = a.res[a.alias[p.k++]];
                const double x = (double)r.x / (double)r.y;                               // metrics.py:221
                if (x >= best) { best = x; best_len = r.y; }                              // sorted(...)[-1] (metrics.py:223)
            }
            p.num = p.num + best * (double)best_len;                                      // statistics.py:22
            p.den += best_len;
        }
    }
}

// The visits of one bitmap word's shared bits, in ascending order.  sw / tw: the source's and the target's word, by value; bs / bt:
// the entry index of the first set bit of either (rankpre).
template <int MODE>
__device__ __forceinline__ void pc_walk_word(const PcDev& d, const PcWalkArgs& a, PcAccOf<MODE>& acc, uint64_t sw, uint64_t tw, uint32_t bs, uint32_t bt,
                                             unsigned long long& cells, unsigned long long& rbytes) {
    uint64_t x = sw & tw;
    while (x) {
        const int b = __ffsll((long long)x) - 1;
        x &= x - 1;
        const uint64_t below = (1ULL << b) - 1;
        pc_visit<MODE>(d, a, acc, bs + __popcll(sw & below), bt + __popcll(tw & below), cells, rbytes);
    }
}

// The value of pair (s, t), s < t, from what the visits left (GCS / JC: from |S n T|, which k_walk_rows counts into acc.k).
template <int MODE>
__device__ __forceinline__ double pc_walk_value(const PcDev& d, const PcPairAcc& acc, int s, int t, int as_distance) {
    if (MODE == PCW_GCS) return pc_set_value<PC_GCS>((int)acc.k, d.nph[s] + d.nph[t], as_distance);
    if (MODE == PCW_JC) return pc_set_value<PC_JC>((int)acc.k, d.nph[s] + d.nph[t], as_distance);
    if (MODE == PCW_POCP) return pc_finish(acc.any ? (double)acc.cons / (double)(d.ngen[s] + d.ngen[t]) : 0.0, as_distance);   // metrics.py:104-110
    double aai = 0.0, af = 0.0;
    if (MODE == PCW_AAI || MODE == PCW_PEQ) aai = acc.any ? acc.num / (double)acc.den : 0.0;                          // metrics.py:227
    if (MODE == PCW_AF || MODE == PCW_PEQ) af = acc.any ? (double)acc.cons / (double)(d.tlen[s] + d.tlen[t]) : 0.0;   // metrics.py:149-152
    if (MODE == PCW_AAI) return pc_finish(aai, as_distance);
    if (MODE == PCW_AF) return pc_finish(af, as_distance);
    return pc_finish(pc_round6(af) * pc_round6(aai), as_distance);                                                    // metrics.py:247-253
}

// JOINT's epilogue: every metric of the launch's set to element `at` of its own array.  Each value is pc_walk_value of that metric's
// own mode over that mode's view of the sums (k = |S n T| for GCS / JC, cons = the gene count for POCP, PEQ's own for AF / AAI / PEQ):
// the expressions of the single-metric fills, called, so the values are theirs bit for bit.
__device__ __forceinline__ void pc_walk_joint_values(const PcDev& d, const PcJointArgs& a, const PcJointAcc& acc, int s, int t, int64_t at) {
    PcPairAcc v = acc;
    if (a.mask & (1u << PC_AF)) a.jout[PC_AF][at] = pc_walk_value<PCW_AF>(d, v, s, t, a.as_distance);
    if (a.mask & (1u << PC_AAI)) a.jout[PC_AAI][at] = pc_walk_value<PCW_AAI>(d, v, s, t, a.as_distance);
    if (a.mask & (1u << PC_PEQ)) a.jout[PC_PEQ][at] = pc_walk_value<PCW_PEQ>(d, v, s, t, a.as_distance);
    v.cons = acc.genes;
    if (a.mask & (1u << PC_POCP)) a.jout[PC_POCP][at] = pc_walk_value<PCW_POCP>(d, v, s, t, a.as_distance);
    v.k = acc.shared;
    if (a.mask & (1u << PC_GCS)) a.jout[PC_GCS][at] = pc_walk_value<PCW_GCS>(d, v, s, t, a.as_distance);
    if (a.mask & (1u << PC_JC)) a.jout[PC_JC][at] = pc_walk_value<PCW_JC>(d, v, s, t, a.as_distance);
}
// ... and a pair list's diagonal entry: 1 - as_distance in every array of the set (matrix.py:467-468)
__device__ __forceinline__ void pc_walk_joint_diagonal(const PcJointArgs& a, int64_t at) {
#pragma unroll
    for (int m = 0; m < 6; ++m) if (a.mask & (1u << m)) a.jout[m][at] = a.as_distance ? 0.0 : 1.0;
}

// COUNT's tail: the workgroup's alignments, DP cells and residue bytes -> totals[0..2] (wave shuffle, LDS atomics, one global atomic each)
__device__ __forceinline__ void pc_walk_totals(unsigned long long* red, unsigned long long* totals, unsigned long long nal,
                                               unsigned long long cells, unsigned long long rbytes) {
    for (int o = 32; o > 0; o >>= 1) {
        nal += __shfl_down(nal, o); cells += __shfl_down(cells, o); rbytes += __shfl_down(rbytes, o);
    }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&red[0], nal); atomicAdd(&red[1], cells); atomicAdd(&red[2], rbytes); }
    __syncthreads();
    if (threadIdx.x < 3 && red[threadIdx.x]) atomicAdd(&totals[threadIdx.x], red[threadIdx.x]);
}

// Stage one chunk of bitmap words of the tile's 32 source rows and 32 target rows.
__device__ __forceinline__ void pc_stage_tile(const PcDev& d, const PcShard& sh, int s0, int k0, int w0, int wn,
                                              uint64_t (*rs)[WCH + 1], uint64_t (*rt)[WCH + 1]) {
    for (int r = threadIdx.x >> 5; r < TS; r += 8) {
        int s = s0 + r, k = k0 + r;
        const uint64_t* ps = s < d.N ? d.bitmap + (int64_t)s * d.Wstride + w0 : nullptr;
        const uint64_t* pt = k < sh.nown ? d.bitmap + (int64_t)sh.owned[k] * d.Wstride + w0 : nullptr;
        for (int w = threadIdx.x & 31; w < wn; w += 32) {
            rs[r][w] = ps ? ps[w] : 0ULL;
            rt[r][w] = pt ? pt[w] : 0ULL;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_walk(PcDev d, PcShard sh, PcArgsOf<MODE> a) {
    __shared__ uint64_t rs[TS][WCH + 1];
    __shared__ uint64_t rt[TS][WCH + 1];
    __shared__ unsigned long long red[3];
    int tile_x, tile_y;
    if (!pc_tile_of_block((d.N + TS - 1) / TS, (sh.nown + TS - 1) / TS, tile_x, tile_y)) return;
    const int s0 = tile_x * TS, k0 = tile_y * TS;
    const int klast = min(k0 + TS, sh.nown) - 1;
    if (s0 >= sh.owned[klast]) return;
    const int f = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int cond = a.condensed;
    PcAccOf<MODE> acc[4];
    int ss[4], kk[4], tt[4]; bool ok[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int ls = cond ? q + 8 * m : f, lt = cond ? f : q + 8 * m;
        ss[m] = s0 + ls; kk[m] = k0 + lt;
        ok[m] = ss[m] < d.N && kk[m] < sh.nown;
        tt[m] = ok[m] ? sh.owned[kk[m]] : 0;
        ok[m] = ok[m] && ss[m] < tt[m];
        acc[m].reset();
        if (ok[m] && pc_walks_slots(MODE)) acc[m].k = a.off[sh.lbase[kk[m]] + ss[m]];
    }
    unsigned long long cells = 0, rbytes = 0;
    if (MODE == PCW_COUNT) { if (threadIdx.x < 3) red[threadIdx.x] = 0; }

    for (int w0 = 0; w0 < d.Wb; w0 += WCH) {
        const int wn = min(WCH, d.Wb - w0);
        if (w0) __syncthreads();
        pc_stage_tile(d, sh, s0, k0, w0, wn, rs, rt);
        __syncthreads();
        // A pair shares ~3 of its ~80 bitmap words, but some lane of the wave has a hit in almost every word: visiting
        // inside the word scan would run the (divergent, memory-touching) visit body ~70 times per pair slot.  So the
        // scan only records which words intersect (branch-free, one 32-bit mask per pair: WCH == 32), and the visits then
        // loop over the set bits of that mask -- as many iterations as the busiest lane has shared words.  Order stays
        // ascending.  A thread's four pairs share one row (t under condensed output, s otherwise): its word is read once.
        uint32_t nz[4] = {0u, 0u, 0u, 0u};
        for (int i = 0; i < wn; ++i) {
            const uint64_t common = cond ? rt[f][i] : rs[f][i];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint64_t other = cond ? rs[q + 8 * m][i] : rt[q + 8 * m][i];
                nz[m] |= ((other & common) != 0 ? 1u : 0u) << i;
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (!ok[m]) continue;
            const int ls = ss[m] - s0, lt = kk[m] - k0;
            const uint32_t* rps = d.rankpre + (int64_t)ss[m] * d.Wb + w0;
            const uint32_t* rpt = d.rankpre + (int64_t)tt[m] * d.Wb + w0;
            uint32_t todo = nz[m];
            while (todo) {
                const int w = __ffs((int)todo) - 1;
                todo &= todo - 1;
                pc_walk_word<MODE>(d, a, acc[m], rs[ls][w], rt[lt][w], rps[w], rpt[w], cells, rbytes);
            }
        }
    }

    if (MODE == PCW_COUNT) {
        unsigned long long nal = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) if (ok[m]) {
            if (a.na) a.na[sh.lbase[kk[m]] + ss[m]] = acc[m].k;
            if (a.cost_t && acc[m].den) atomicAdd(&a.cost_t[tt[m]], (unsigned long long)acc[m].den);
            if (a.aln_t && acc[m].k) atomicAdd(&a.aln_t[tt[m]], (unsigned long long)acc[m].k);
            nal += acc[m].k;
        }
        pc_walk_totals(red, a.totals, nal, cells, rbytes);
        return;
    }
    if (MODE == PCW_ENUM) return;

#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (!ok[m]) continue;
        const int64_t at = pc_out_index(d, sh, ss[m], tt[m], kk[m], cond);
        if constexpr (MODE == PCW_JOINT) pc_walk_joint_values(d, a, acc[m], ss[m], tt[m], at);
        else a.out[at] = pc_walk_value<MODE>(d, acc[m], ss[m], tt[m], a.as_distance);
    }
}

int pc_launch_walk(int mode, const PcDev& d, const PcShard& sh, const PcWalkArgs& a, hipStream_t st, pc_set_shape* shape_out) {
    pc_set_shape shp;
    pc_set_shape_of(K_WALKER, mode == PCW_POCP ? PC_POCP : PC_AF, d.N, sh.nown, d.Wb, d.sp_W, d.n_cu, 0, PcSetKnobs{0, 0, 0}, &shp);
    if (shape_out) *shape_out = shp;
    if (sh.nown <= 0 || d.N <= 1) return PC_OK;
    dim3 grid((unsigned)shp.grid), block(256);
    if (!pc_dispatch<PCW_POCP, PCW_AF, PCW_COUNT, PCW_ENUM, PCW_AAI, PCW_PEQ>(mode, [&](auto m) { hipLaunchKernelGGL(k_walk<decltype(m)::value>, grid, block, 0, st, d, sh, a); })) {
        pc_set_error("pc_launch_walk: bad mode %d", mode); return PC_ERR_ARG;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_walk launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// k_walk<PCW_JOINT>: the condensed triangle of the shard's pairs, every array of the set at pc_out_index(..., cond = 1)
int pc_launch_walk_joint(const PcDev& d, const PcShard& sh, const PcJointArgs& a, hipStream_t st) {
    if (!a.condensed) { pc_set_error("pc_launch_walk_joint: condensed output only"); return PC_ERR_ARG; }
    if (sh.nown <= 0 || d.N <= 1) return PC_OK;
    dim3 grid(pc_tile_grid((d.N + TS - 1) / TS, (sh.nown + TS - 1) / TS)), block(256);        // (the walker's grid: pc_set_shape_of(K_WALKER))
    hipLaunchKernelGGL(k_walk<PCW_JOINT>, grid, block, 0, st, d, sh, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_walk launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// ---------------------------------------------------------------------------------
// The walker over a ROWS domain (pc_fill_rows): the pairs {q, g} of the query genomes q = rows[k], kb <= k < ke, with every
// other genome g.  The reference has the container half of this (SymMatrix.append_node, matrix.py:169-213) and nothing that
// produces its values; a pair runs here exactly as in the whole fill: s = min(q, g) is the reference's `source`, t = max(q, g)
// its `target` (matrix.py:479-486; aai is not symmetric: a query is the source of some of its pairs and the target of others).
//
// A tile is TS query rows x TS genomes.  Lanes run over g, so the stores into out[k * N + g] are coalesced and a thread's four
// slots (rows q + 8 m of the tile) share one genome: its bitmap word is read once per scanned word, from 32 distinct LDS rows of
// odd stride (conflict free), the query's word is a broadcast.  What k_walk's comments say on the word scan (record which words
// intersect, visit afterwards) and on the XCD-aware tile order holds unchanged; no tile is skipped, the domain is a rectangle.
// Slot (k, g) is live iff g != q and not (g is a query itself and g < q): a pair of two queries belongs to the slot of the
// smaller one, which also writes the mirror cell out[row_of[g] * N + q].  The slot g == q writes the diagonal, 1 - as_distance
// (matrix.py:467-468).  Slot arrays (na, off) are [ke - kb][N]: slot (k - kb) * N + g; dead slots count zero alignments.
// COUNT also sums a row's alignments into aln_t[k] (where a rows fill is cut into chunks); ENUM emits k_walk's keys, so the
// sort, k_unique, the task builders and the alignment launches do not know which domain they serve.  GCS / JC count the shared
// phams in the word scan itself and finish through pc_set_value's division, the tile kernels' own (table-free) epilogue.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void pc_stage_tile_rows(const PcDev& d, const PcRows& rw, int g0, int k0, int ke, int w0, int wn,
                                                   uint64_t (*rg)[WCH + 1], uint64_t (*rq)[WCH + 1]) {
    for (int r = threadIdx.x >> 5; r < TS; r += 8) {
        const int g = g0 + r, k = k0 + r;
        const uint64_t* pg = g < d.N ? d.bitmap + (int64_t)g * d.Wstride + w0 : nullptr;
        const uint64_t* pq = k < ke ? d.bitmap + (int64_t)rw.rows[k] * d.Wstride + w0 : nullptr;
        for (int w = threadIdx.x & 31; w < wn; w += 32) {
            rg[r][w] = pg ? pg[w] : 0ULL;
            rq[r][w] = pq ? pq[w] : 0ULL;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_walk_rows(PcDev d, PcRows rw, int kb, int ke, PcWalkArgs a) {
    constexpr bool SETS = MODE == PCW_GCS || MODE == PCW_JC;                        // shared-pham counts: no visit
    constexpr bool SLOTS = MODE == PCW_ENUM || MODE == PCW_AAI || MODE == PCW_PEQ;  // walks the pair's alignment slots
    __shared__ uint64_t rg[TS][WCH + 1];                    // the tile's genomes g
    __shared__ uint64_t rq[TS][WCH + 1];                    // the tile's query rows
    __shared__ unsigned long long red[3];
    int tile_x, tile_y;
    if (!pc_tile_of_block((d.N + TS - 1) / TS, (ke - kb + TS - 1) / TS, tile_x, tile_y)) return;
    const int g0 = tile_x * TS, k0 = kb + tile_y * TS;
    const int f = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int g = g0 + f;
    const int g_row = g < d.N ? rw.row_of[g] : -1;          // g's own query row, or -1
    PcPairAcc acc[4];
    int kk[4], qq[4]; bool ok[4], diag[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        kk[m] = k0 + r0 + 8 * m;
        const bool in = g < d.N && kk[m] < ke;
        qq[m] = in ? rw.rows[kk[m]] : 0;
        diag[m] = in && g == qq[m];
        ok[m] = in && g != qq[m] && !(g_row >= 0 && g < qq[m]);
        acc[m].reset();
        if (ok[m] && SLOTS) acc[m].k = a.off[(int64_t)(kk[m] - kb) * d.N + g];
    }
    unsigned long long cells = 0, rbytes = 0;
    if (MODE == PCW_COUNT) { if (threadIdx.x < 3) red[threadIdx.x] = 0; }

    for (int w0 = 0; w0 < d.Wb; w0 += WCH) {
        const int wn = min(WCH, d.Wb - w0);
        if (w0) __syncthreads();
        pc_stage_tile_rows(d, rw, g0, k0, ke, w0, wn, rg, rq);
        __syncthreads();
        uint32_t nz[4] = {0u, 0u, 0u, 0u};
        for (int i = 0; i < wn; ++i) {
            const uint64_t common = rg[f][i];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint64_t both = rq[r0 + 8 * m][i] & common;
                if (SETS) acc[m].k += (uint32_t)__popcll(both);
                else nz[m] |= (both != 0 ? 1u : 0u) << i;
            }
        }
        if constexpr (!SETS) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!ok[m]) continue;
                const bool q_is_source = qq[m] < g;
                const int s = q_is_source ? qq[m] : g, t = q_is_source ? g : qq[m];
                const uint32_t* rps = d.rankpre + (int64_t)s * d.Wb + w0;
                const uint32_t* rpt = d.rankpre + (int64_t)t * d.Wb + w0;
                uint32_t todo = nz[m];
                while (todo) {
                    const int w = __ffs((int)todo) - 1;
                    todo &= todo - 1;
                    const uint64_t qw = rq[r0 + 8 * m][w], gw = rg[f][w];
                    pc_walk_word<MODE>(d, a, acc[m], q_is_source ? qw : gw, q_is_source ? gw : qw, rps[w], rpt[w], cells, rbytes);
                }
            }
        }
    }

    if (MODE == PCW_COUNT) {
        unsigned long long nal = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t n = ok[m] ? acc[m].k : 0u;
            if (ok[m] && a.na) a.na[(int64_t)(kk[m] - kb) * d.N + g] = n;
            nal += n;
            if (a.aln_t) {                                                // the 32 lanes of a half-wave hold one row's slots: one add per tile and row
                unsigned long long row_sum = n;
                for (int o = 16; o > 0; o >>= 1) row_sum += __shfl_down(row_sum, o, 32);
                if (f == 0 && row_sum && kk[m] < ke) atomicAdd(&a.aln_t[kk[m]], row_sum);
            }
        }
        pc_walk_totals(red, a.totals, nal, cells, rbytes);
        return;
    }
    if (MODE == PCW_ENUM) return;

#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (diag[m]) a.out[(int64_t)kk[m] * d.N + g] = a.as_distance ? 0.0 : 1.0;
        if (!ok[m]) continue;
        const int q = qq[m];
        const double v = pc_walk_value<MODE>(d, acc[m], q < g ? q : g, q < g ? g : q, a.as_distance);
        a.out[(int64_t)kk[m] * d.N + g] = v;
        if (g_row >= 0) a.out[(int64_t)g_row * d.N + q] = v;               // two queries: the mirror cell of the larger one's row
    }
}

int pc_launch_walk_rows(int mode, const PcDev& d, const PcRows& rw, int kb, int ke, const PcWalkArgs& a, hipStream_t st) {
    if (kb < 0 || ke > rw.nrows || kb > ke) { pc_set_error("pc_launch_walk_rows: rows [%d, %d) of %d", kb, ke, rw.nrows); return PC_ERR_ARG; }
    if (ke == kb || d.N < 1) return PC_OK;
    dim3 grid(pc_tile_grid((d.N + TS - 1) / TS, (ke - kb + TS - 1) / TS)), block(256);
    if (!pc_dispatch<PCW_GCS, PCW_JC, PCW_POCP, PCW_AF, PCW_COUNT, PCW_ENUM, PCW_AAI, PCW_PEQ>(
            mode, [&](auto m) { hipLaunchKernelGGL(k_walk_rows<decltype(m)::value>, grid, block, 0, st, d, rw, kb, ke, a); })) {
        pc_set_error("pc_launch_walk_rows: bad mode %d", mode); return PC_ERR_ARG;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_walk_rows launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// ---------------------------------------------------------------------------------
// The walker over a GROUPS domain (pc_fill_groups): every pair of two genomes that lie in the same group of a caller-given family of
// groups -- a block diagonal, sum of n_c^2 cells instead of N^2.  The reference reads such blocks out of the dense matrix
// (SymMatrix.extract_submatrix, matrix.py:155-167); here they are filled alone.  The groups' members are laid end to end as M
// positions; members ascend inside a group, so for two positions p < q of one group genome[p] < genome[q]: the row's genome is the
// reference's `source`, the column's its `target` (matrix.py:479-486), the whole fill's orientation.
//
// Tiles are TS x TS over POSITIONS, not per group, so many small groups share a tile; the host lists the live ones -- row block a,
// column block b >= a, some slot of the tile live: a band along the diagonal -- sorted by a, and a workgroup takes tile tb +
// blockIdx.x of that list (neighbouring workgroups then share rows, which is all the affinity a band has to offer).  Slot (p, q) is
// live iff p < q < pos_end[p]; its index in out, and (less slot_base) in the slot arrays na / off, is pos_rowbase[p] + q - p - 1:
// a group's condensed triangle, the groups' triangles end to end, no dead slot.  Lanes run over q: a row's stores are contiguous
// and a thread's four slots (rows r0 + 8 m) share the column genome, whose word is read once per scanned word from 32 LDS rows of
// odd stride; the row's word is a broadcast.  What k_walk says on the word scan holds unchanged.  COUNT sums a workgroup's
// alignments into aln_t[a], its ROW BLOCK (where a groups fill is cut: a range of row blocks is a range of the tile list and of
// the slots); ENUM emits k_walk's keys.  GCS / JC count in the word scan, as in k_walk_rows.
// ---------------------------------------------------------------------------------
static_assert(PC_GROUP_TILE == TS, "the host lists the groups walker's tiles by PC_GROUP_TILE");
__device__ __forceinline__ void pc_stage_tile_groups(const PcDev& d, const PcGroups& gr, int64_t p0, int64_t q0, int w0, int wn,
                                                     uint64_t (*rp)[WCH + 1], uint64_t (*rq)[WCH + 1]) {
    for (int r = threadIdx.x >> 5; r < TS; r += 8) {
        const int64_t p = p0 + r, q = q0 + r;
        const uint64_t* pp = p < gr.M ? d.bitmap + (int64_t)gr.pos_genome[p] * d.Wstride + w0 : nullptr;
        const uint64_t* pq = q < gr.M ? d.bitmap + (int64_t)gr.pos_genome[q] * d.Wstride + w0 : nullptr;
        for (int w = threadIdx.x & 31; w < wn; w += 32) {
            rp[r][w] = pp ? pp[w] : 0ULL;
            rq[r][w] = pq ? pq[w] : 0ULL;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_walk_groups(PcDev d, PcGroups gr, int64_t tb, PcWalkArgs a) {
    constexpr bool SETS = MODE == PCW_GCS || MODE == PCW_JC;                        // shared-pham counts: no visit
    constexpr bool SLOTS = MODE == PCW_ENUM || MODE == PCW_AAI || MODE == PCW_PEQ;  // walks the pair's alignment slots
    __shared__ uint64_t rp[TS][WCH + 1];                    // the tile's row positions p (sources)
    __shared__ uint64_t rq[TS][WCH + 1];                    // the tile's column positions q (targets)
    __shared__ unsigned long long red[3];
    const int64_t tile = tb + blockIdx.x;
    const int row_block = gr.tile_row[tile];
    const int64_t p0 = (int64_t)row_block * TS, q0 = (int64_t)gr.tile_col[tile] * TS;
    const int f = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int64_t q = q0 + f;
    const bool q_in = q < gr.M;
    const int t = q_in ? gr.pos_genome[q] : 0;
    PcPairAcc acc[4];
    int ss[4]; int64_t slot[4]; bool ok[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int64_t p = p0 + r0 + 8 * m;
        ok[m] = q_in && p < q && q < gr.pos_end[p];          // (p < q < M: pos_end[p] is in bounds)
        ss[m] = ok[m] ? gr.pos_genome[p] : 0;
        slot[m] = ok[m] ? gr.pos_rowbase[p] + (q - p - 1) : 0;
        acc[m].reset();
        if (ok[m] && SLOTS) acc[m].k = a.off[slot[m] - gr.slot_base];
    }
    unsigned long long cells = 0, rbytes = 0;
    if (MODE == PCW_COUNT) { if (threadIdx.x < 3) red[threadIdx.x] = 0; }

    for (int w0 = 0; w0 < d.Wb; w0 += WCH) {
        const int wn = min(WCH, d.Wb - w0);
        if (w0) __syncthreads();
        pc_stage_tile_groups(d, gr, p0, q0, w0, wn, rp, rq);
        __syncthreads();
        uint32_t nz[4] = {0u, 0u, 0u, 0u};
        for (int i = 0; i < wn; ++i) {
            const uint64_t common = rq[f][i];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint64_t both = rp[r0 + 8 * m][i] & common;
                if (SETS) acc[m].k += (uint32_t)__popcll(both);
                else nz[m] |= (both != 0 ? 1u : 0u) << i;
            }
        }
        if constexpr (!SETS) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!ok[m]) continue;
                const uint32_t* rps = d.rankpre + (int64_t)ss[m] * d.Wb + w0;
                const uint32_t* rpt = d.rankpre + (int64_t)t * d.Wb + w0;
                uint32_t todo = nz[m];
                while (todo) {
                    const int w = __ffs((int)todo) - 1;
                    todo &= todo - 1;
                    pc_walk_word<MODE>(d, a, acc[m], rp[r0 + 8 * m][w], rq[f][w], rps[w], rpt[w], cells, rbytes);
                }
            }
        }
    }

    if (MODE == PCW_COUNT) {
        unsigned long long nal = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (!ok[m]) continue;
            if (a.na) a.na[slot[m] - gr.slot_base] = acc[m].k;
            nal += acc[m].k;
        }
        pc_walk_totals(red, a.totals, nal, cells, rbytes);
        if (a.aln_t && threadIdx.x == 0 && red[0]) atomicAdd(&a.aln_t[row_block], red[0]);     // (red[] is final behind the barrier of pc_walk_totals)
        return;
    }
    if (MODE == PCW_ENUM) return;

#pragma unroll
    for (int m = 0; m < 4; ++m)
        if (ok[m]) a.out[slot[m]] = pc_walk_value<MODE>(d, acc[m], ss[m], t, a.as_distance);
}

int pc_launch_walk_groups(int mode, const PcDev& d, const PcGroups& gr, int64_t tb, int64_t te, const PcWalkArgs& a, hipStream_t st) {
    if (tb < 0 || tb > te || te - tb > 0x7fffffffLL) { pc_set_error("pc_launch_walk_groups: tiles [%lld, %lld)", (long long)tb, (long long)te); return PC_ERR_ARG; }
    if (te == tb || gr.M < 2) return PC_OK;
    dim3 grid((unsigned)(te - tb)), block(256);
    if (!pc_dispatch<PCW_GCS, PCW_JC, PCW_POCP, PCW_AF, PCW_COUNT, PCW_ENUM, PCW_AAI, PCW_PEQ>(
            mode, [&](auto m) { hipLaunchKernelGGL(k_walk_groups<decltype(m)::value>, grid, block, 0, st, d, gr, tb, a); })) {
        pc_set_error("pc_launch_walk_groups: bad mode %d", mode); return PC_ERR_ARG;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_walk_groups launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// ---------------------------------------------------------------------------------
// The walker over a PAIRS domain (pc_fill_pairs): a flat list of pairs the caller names, the reference's most basic interface,
// METRICS[metric](source, target), for many pairs in one call.  The host sorts the list on the device by (target, source)
// (k_pair_keys -> pc_sort_pairs -> k_pair_split), so slot i holds source src[i], target tgt[i] and the caller's position at[i]:
// neighbouring lanes mostly share their target row, and entries listed twice sit side by side.
//
// The list is ORIENTED: src[i] is the reference's `source` and tgt[i] its `target` whatever their index order.  pc_visit decides
// the anchor from the two entries it is handed (fewer genes, tie -> source) and pc_walk_value reads per-genome sums only, so the two
// genomes pass through as given: with src < tgt the value is the whole fill's cell bit for bit, with src > tgt (aai, aai_ppos, peq)
// it is the other orientation, which no other fill computes.  src == tgt is the diagonal, 1 - as_distance (matrix.py:467-468): a
// dead slot, no visit, no alignment.
//
// A workgroup takes PC_PAIR_BLOCK consecutive slots, one lane per slot.  A list has no tile to amortise an LDS stage over: each
// lane reads the words of its two rows straight from the bitmap (in a sorted wave the target's word is mostly one address for all
// lanes; a source row is one 128-byte line per 16 words).  The two-step scan of the other walkers holds: which of up to WCH words
// intersect goes into one 32-bit mask, the visits follow, so a wave stays together through the word loop.  Slot arrays (na, off)
// hold the launch's slots, slot - slot_base; COUNT adds a workgroup's alignments into aln_t[block] (where a pair-list fill is cut);
// ENUM emits k_walk's keys.  GCS / JC count in the word scan, as in k_walk_rows.
// ---------------------------------------------------------------------------------
static_assert(PC_PAIR_BLOCK == 256, "k_walk_pairs runs one lane per slot of a block");
template <int MODE>
__global__ __launch_bounds__(256) void k_walk_pairs(PcDev d, PcPairs pr, int64_t bb, PcArgsOf<MODE> a) {
    constexpr bool SETS = MODE == PCW_GCS || MODE == PCW_JC;                        // shared-pham counts: no visit
    constexpr bool SLOTS = pc_walks_slots(MODE);                                    // walks the pair's alignment slots
    __shared__ unsigned long long red[3];
    const int64_t block = bb + blockIdx.x;
    const int64_t slot = block * PC_PAIR_BLOCK + threadIdx.x;
    const bool in = slot < pr.L;
    const int s = in ? pr.src[slot] : 0, t = in ? pr.tgt[slot] : 0;                 // (a lane past the list scans genome 0 against itself, and visits nothing)
    const bool ok = in && s != t;
    PcAccOf<MODE> acc; acc.reset();
    if (ok && SLOTS) acc.k = a.off[slot - pr.slot_base];
    unsigned long long cells = 0, rbytes = 0;
    if (MODE == PCW_COUNT) { if (threadIdx.x < 3) red[threadIdx.x] = 0; __syncthreads(); }

    const uint64_t* const ps = d.bitmap + (int64_t)s * d.Wstride;
    const uint64_t* const pt = d.bitmap + (int64_t)t * d.Wstride;
    const uint32_t* const rps = d.rankpre + (int64_t)s * d.Wb;
    const uint32_t* const rpt = d.rankpre + (int64_t)t * d.Wb;
    for (int w0 = 0; w0 < d.Wb; w0 += WCH) {
        const int wn = min(WCH, d.Wb - w0);
        uint32_t nz = 0u;
        for (int i = 0; i < wn; ++i) {
            const uint64_t both = ps[w0 + i] & pt[w0 + i];
            if (SETS) acc.k += (uint32_t)__popcll(both);
            else nz |= (both != 0 ? 1u : 0u) << i;
        }
        if constexpr (!SETS) {
            uint32_t todo = ok ? nz : 0u;
            while (todo) {
                const int w = w0 + __ffs((int)todo) - 1;
                todo &= todo - 1;
                pc_walk_word<MODE>(d, a, acc, ps[w], pt[w], rps[w], rpt[w], cells, rbytes);
            }
        }
    }

    if (MODE == PCW_COUNT) {
        const uint32_t n = ok ? acc.k : 0u;
        if (ok && a.na) a.na[slot - pr.slot_base] = n;
        pc_walk_totals(red, a.totals, n, cells, rbytes);
        if (a.aln_t && threadIdx.x == 0 && red[0]) atomicAdd(&a.aln_t[block], red[0]);        // (red[] is final behind the barrier of pc_walk_totals)
        return;
    }
    if (MODE == PCW_ENUM) return;
    if (!in) return;
    if constexpr (MODE == PCW_JOINT) {
        if (ok) pc_walk_joint_values(d, a, acc, s, t, pr.at[slot]);
        else pc_walk_joint_diagonal(a, pr.at[slot]);
    } else a.out[pr.at[slot]] = ok ? pc_walk_value<MODE>(d, acc, s, t, a.as_distance) : (a.as_distance ? 0.0 : 1.0);
}

int pc_launch_walk_pairs(int mode, const PcDev& d, const PcPairs& pr, int64_t bb, int64_t be, const PcWalkArgs& a, hipStream_t st) {
    const int64_t nb = (pr.L + PC_PAIR_BLOCK - 1) / PC_PAIR_BLOCK;
    if (bb < 0 || bb > be || be > nb || be - bb > 0x7fffffffLL) { pc_set_error("pc_launch_walk_pairs: blocks [%lld, %lld) of %lld", (long long)bb, (long long)be, (long long)nb); return PC_ERR_ARG; }
    if (be == bb || d.N < 1) return PC_OK;
    dim3 grid((unsigned)(be - bb)), block(PC_PAIR_BLOCK);
    if (!pc_dispatch<PCW_GCS, PCW_JC, PCW_POCP, PCW_AF, PCW_COUNT, PCW_ENUM, PCW_AAI, PCW_PEQ>(
            mode, [&](auto m) { hipLaunchKernelGGL(k_walk_pairs<decltype(m)::value>, grid, block, 0, st, d, pr, bb, a); })) {
        pc_set_error("pc_launch_walk_pairs: bad mode %d", mode); return PC_ERR_ARG;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_walk_pairs launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

int pc_launch_walk_pairs_joint(const PcDev& d, const PcPairs& pr, int64_t bb, int64_t be, const PcJointArgs& a, hipStream_t st) {
    const int64_t nb = (pr.L + PC_PAIR_BLOCK - 1) / PC_PAIR_BLOCK;
    if (bb < 0 || bb > be || be > nb || be - bb > 0x7fffffffLL) { pc_set_error("pc_launch_walk_pairs_joint: blocks [%lld, %lld) of %lld", (long long)bb, (long long)be, (long long)nb); return PC_ERR_ARG; }
    if (be == bb || d.N < 1) return PC_OK;
    dim3 grid((unsigned)(be - bb)), block(PC_PAIR_BLOCK);
    hipLaunchKernelGGL(k_walk_pairs<PCW_JOINT>, grid, block, 0, st, d, pr, bb, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_walk_pairs launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// The sort of a pair list, around pc_sort_pairs: entry i -> key tgt << 32 | src, value i; and the sorted keys back into src / tgt.
__global__ __launch_bounds__(256) void k_pair_keys(const int32_t* __restrict__ src, const int32_t* __restrict__ tgt, unsigned long long* __restrict__ key,
                                                   uint32_t* __restrict__ val, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = ((unsigned long long)(uint32_t)tgt[i] << 32) | (unsigned long long)(uint32_t)src[i];
    val[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_pair_split(const unsigned long long* __restrict__ key, int32_t* __restrict__ src, int32_t* __restrict__ tgt, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    src[i] = (int32_t)(uint32_t)(k & 0xffffffffull);
    tgt[i] = (int32_t)(uint32_t)(k >> 32);
}
int pc_launch_pair_keys(const int32_t* src, const int32_t* tgt, unsigned long long* key, uint32_t* val, int64_t n, hipStream_t st) {
    if (n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_pair_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, tgt, key, val, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_pair_keys launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
int pc_launch_pair_split(const unsigned long long* key, int32_t* src, int32_t* tgt, int64_t n, hipStream_t st) {
    if (n <= 0) return PC_OK;
    hipLaunchKernelGGL(k_pair_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, key, src, tgt, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_pair_split launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
