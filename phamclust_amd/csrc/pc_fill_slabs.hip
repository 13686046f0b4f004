// pc_fill_slabs.hip -- the fills of libphamclust_hip.so that walk the matrix slab by slab and deliver what a threshold leaves of it:
// pc_fill_edges (the passing pairs as an edge list; pc_fill_edges_bars: under a bar per genome) and pc_fill_components (their connected components), with pc_last_edge_times and
// pc_last_component_times -- and, on the same walk without a threshold, pc_fill_nearest (every genome's k best neighbours) with
// pc_last_nearest_times (beside it pc_nearest_of_pairs, the same lists from a caller's pair list: no walk), pc_fill_tree (the single-linkage dendrogram as N - 1 edges) with pc_last_tree_times / pc_last_tree_rounds, and
// pc_fill_between (the count, sum, minimum and maximum of the pair values between every two groups of a partition) with pc_last_between_times,
// pc_fill_affinity (the sum, minimum and maximum of every genome's pair values to every group) with pc_last_affinity_times,
// pc_fill_hist (the exact histogram of all pair values, split by a partition into within and between) with pc_last_hist_times.
// Each fill is described once (PcEdgesFill, PcComponentsFill, PcNearestFill, PcTreeFill, PcBetweenFill, PcAffinityFill, PcHistFill: begin, slab, end, and what several
// devices ship and merge; declared in pc_host.h) and run by one driver, pc_slab_fill<Fill>: check -> begin -> walk [0, N) -> end.
// multi_slab_fill<Fill> (pc_multi.hip) runs the same description on a stretch of targets per device.  An entry point sets the call's
// own fields of a PcSlabRun and hands a driver to pc_slab_call<Fill> (pc_host.h), which clears and delivers the outputs.  Host only.
// pc_fill_rows_edges / pc_fill_rows_components / pc_fill_rows_tree / pc_fill_rows_nearest / pc_fill_rows_affinity / pc_fill_rows_between / pc_fill_rows_hist (at the end of the file) grow a stored result by new genomes: the same
// descriptions, seeded, over a walk of the new genomes' rows instead of the triangle (pc_rows_slab_fill<Fill>, rows_walk): slab() takes
// either slab's pair domain.
//
// The walk they share goes over successive contiguous ranges of target genomes ("slabs": pc_chunk_plan over count[t] = t under
// slab_bytes / 8 pairs, at most 2^31-1 so that u32 counts and offsets do); each range is installed as a PcShard (owned = t0 .. t1-1,
// shard-local layout), filled by fill_impl into the context's slab buffer and handed to the description's slab().  Slabs come in
// ascending target order; one slab is resident at a time.
#include <chrono>
#include <climits>

#include "pc_host.h"

#define PC_EDGE_MAX_PAIRS 0x7fffffffLL

namespace {
// the caller's unsharded state, put back however the call ends (the slab shards live in buffers of their own: b_owned / b_lbase,
// the deal tables, rank / world and the stride are never touched)
struct SlabShardScope {
    pc_ctx* c; PcShard shard; int64_t pairs; std::vector<int32_t> owned; std::vector<int64_t> lbase;
    explicit SlabShardScope(pc_ctx* ctx) : c(ctx), shard(ctx->shard), pairs(ctx->shard_pairs), owned(ctx->h_owned), lbase(ctx->h_lbase) {}
    ~SlabShardScope() { c->shard = shard; c->shard_pairs = pairs; c->h_owned.swap(owned); c->h_lbase.swap(lbase); c->plan.valid = false; }
    SlabShardScope(const SlabShardScope&) = delete; SlabShardScope& operator=(const SlabShardScope&) = delete;
};
}  // namespace

static int64_t pairs_below(int64_t t) { return t * (t - 1) / 2; }           // pairs (s, t'), s < t' < t

// The checks the calls make, in the public calls' order: fill_check's, a nearest-neighbours fill's k (and with it kk: the one place
// that settles it), then outputs (every output pointer is there), the threshold, slab_bytes, and the residues aai / peq need.  Nothing
// but the run is touched.
int pc_slab_check(const pc_ctx* c, PcSlabRun& run, const char* what) {
    int rc = PC_OK;
    const char* who = run.who;
    if ((rc = fill_check(c, who, what, &run.metric, nullptr))) return rc;
    if (run.kind == PC_SLAB_NEAREST) {
        if (run.k < 1) { pc_set_error("%s: k %d", who, run.k); return PC_ERR_ARG; }
        if (run.k > PC_NEAREST_MAX_K) { pc_set_error("%s: k %d is above PC_NEAREST_MAX_K = %d", who, run.k, PC_NEAREST_MAX_K); return PC_ERR_LIMIT; }
        run.kk = std::max(std::min(run.k, c->dev.N - 1), 0);
    }
    if (run.kind == PC_SLAB_BETWEEN || run.kind == PC_SLAB_AFFINITY) {
        if (!run.group) { pc_set_error("%s: group is NULL", who); return PC_ERR_ARG; }
        if (run.n_groups < 1) { pc_set_error("%s: n_groups %d", who, run.n_groups); return PC_ERR_ARG; }
        if (run.n_groups > PC_BETWEEN_MAX_GROUPS) {
            pc_set_error("%s: n_groups %d is above PC_BETWEEN_MAX_GROUPS = %d", who, run.n_groups, PC_BETWEEN_MAX_GROUPS); return PC_ERR_LIMIT;
        }
        const int lowest = run.allow_unlabelled ? -1 : 0;                  // (the rows forms alone: -1 is a member of no group)
        for (int g = 0; g < c->dev.N; ++g)
            if (run.group[g] < lowest || run.group[g] >= run.n_groups) {
                pc_set_error("%s: genome %d has label %d, outside [%d, %d)", who, g, run.group[g], lowest, run.n_groups); return PC_ERR_ARG;
            }
    }
    if (run.kind == PC_SLAB_HIST && run.group) {                            // (no cap on n_groups: the labels are only compared)
        if (run.n_groups < 1) { pc_set_error("%s: n_groups %d", who, run.n_groups); return PC_ERR_ARG; }
        for (int g = 0; g < c->dev.N; ++g)
            if (run.group[g] < 0 || run.group[g] >= run.n_groups) {
                pc_set_error("%s: genome %d has label %d, outside [%d, %d)", who, g, run.group[g], 0, run.n_groups); return PC_ERR_ARG;
            }
    }
    if (run.kind == PC_SLAB_TREE && c->dev.N > PC_TREE_MAX_GENOMES) {
        pc_set_error("%s: %d genomes are above PC_TREE_MAX_GENOMES = %d", who, c->dev.N, PC_TREE_MAX_GENOMES);
        return PC_ERR_LIMIT;
    }
    if (!run.outputs) { pc_set_error("%s: an output pointer is NULL", who); return PC_ERR_ARG; }
    if (run.threshold != run.threshold) { pc_set_error("%s: the threshold is NaN", who); return PC_ERR_ARG; }
    if (run.by_bars) {
        if (!run.bars) { pc_set_error("%s: bar is NULL", who); return PC_ERR_ARG; }
        for (int g = 0; g < c->dev.N; ++g)
            if (run.bars[g] != run.bars[g]) { pc_set_error("%s: the bar of genome %d is NaN", who, g); return PC_ERR_ARG; }
    }
    if (run.slab_bytes < 0) { pc_set_error("%s: slab_bytes %lld", who, (long long)run.slab_bytes); return PC_ERR_ARG; }
    if ((rc = fill_check_residues(c, who, run.metric))) return rc;
    run.as_distance = run.as_distance ? 1 : 0; run.strict = run.strict ? 1 : 0;
    return PC_OK;
}

// Pairs one slab may hold (N > 1).  slab_bytes == 0: the whole domain (`whole` values: the dense triangle; a rows slab fill's n_rows * N),
// or a quarter of what is free now (an aai / peq slab's plan takes its own half) -- so this runs before the call allocates anything of its own.
static int64_t slab_max_pairs(pc_ctx* c, int64_t slab_bytes, int64_t whole) {
    int64_t max_pairs;
    if (slab_bytes > 0) max_pairs = std::max<int64_t>(slab_bytes / 8, 1);
    else {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
        max_pairs = std::min<int64_t>(std::max<int64_t>(whole, 1), std::max<int64_t>((int64_t)((free_b + c->b_edge_slab.cap) / 4 / 8), 1));
    }
    return std::min<int64_t>(max_pairs, PC_EDGE_MAX_PAIRS);
}

// The cut of the targets [ta, tb), 0 <= ta < tb <= N: ranges of targets whose pairs fit the slab -- the chunking rule over count[t] = t
// for the targets of the stretch, so the first range starts at ta -- range starts followed by tb, and the slab buffer sized for the largest.
static int slab_cut(pc_ctx* c, int64_t max_pairs, int ta, int tb, std::vector<int32_t>& cut) {
    const int n = tb - ta;
    std::vector<uint64_t> per_target((size_t)n);
    for (int t = ta; t < tb; ++t) per_target[t - ta] = (uint64_t)t;
    const int nsl = pc_chunk_plan(per_target.data(), n, (uint64_t)max_pairs, nullptr, 0);
    if (nsl < 0) return nsl;
    cut.resize((size_t)nsl + 1);
    int rc = PC_OK;
    if ((rc = pc_chunk_plan(per_target.data(), n, (uint64_t)max_pairs, cut.data(), nsl + 1)) < 0) return rc;
    for (int32_t& x : cut) x += ta;
    int64_t most = 1;
    for (int i = 0; i < nsl; ++i) most = std::max(most, pairs_below(cut[i + 1]) - pairs_below(cut[i]));
    return abi_rc(c->b_edge_slab.ensure((size_t)most * 8));
}
static bool stretch_ok(const pc_ctx* c, const PcSlabRun& run, int ta, int tb) {
    if (0 <= ta && ta <= tb && tb <= c->dev.N) return true;
    pc_set_error("%s: targets [%d, %d) of %d", run.who, ta, tb, c->dev.N);
    return false;
}

// The walk: slab by slab the shard installed, the slab filled (its stats added to *sum when sum != NULL), then hook(slab, Lp, shard) --
// the filled values f64[Lp], and the PcShard that says which pair each is.  A hook that leaves work on the stream which still reads the
// slab or the shard tables says so with mark_work: the walk waits for it before it rewrites the tables (a hook that has drained the
// stream itself costs no wait).  The caller's shard is back in force when this returns, also after a refusal in the middle.
template <class Hook> static int slab_walk(pc_ctx* c, const std::vector<int32_t>& cut, int metric, int as_distance, pc_stats* sum, Hook hook) {
    int rc = PC_OK;
    hipStream_t st = c->stream;
    double* const slab = c->b_edge_slab.as<double>();
    SlabShardScope restore(c);
    std::vector<int32_t> owned; std::vector<int64_t> lbase;
    for (size_t i = 0; i + 1 < cut.size(); ++i) {
        const int t0 = cut[i], t1 = cut[i + 1];
        const int64_t Lp = pairs_below(t1) - pairs_below(t0);
        if (Lp == 0) continue;                                              // (target 0 alone: no pair)
        owned.resize((size_t)(t1 - t0)); lbase.resize((size_t)(t1 - t0) + 1);
        for (int t = t0; t < t1; ++t) { owned[t - t0] = t; lbase[t - t0] = pairs_below(t) - pairs_below(t0); }
        lbase[t1 - t0] = Lp;
        if ((rc = wait_last_work(c, st, false))) return rc;                 // (blocking copies into tables the previous slab's hook may have left in use)
        if ((rc = upload_vec(c->b_edge_owned, owned)) || (rc = upload_vec(c->b_edge_lbase, lbase))) return rc;
        // install the slab's shard as apply_shard installs one: a plan belongs to the shard it was made for, and pick_set_kernel
        // gathers its per-shard inputs (nown, max_block_entries) from what is in force
        c->plan.valid = false;
        c->shard.nown = t1 - t0; c->shard.ident = 0;
        c->shard.owned = c->b_edge_owned.as<int32_t>(); c->shard.lbase = c->b_edge_lbase.as<int64_t>();
        c->h_owned = owned; c->h_lbase = lbase; c->shard_pairs = Lp;
        pc_stats one; memset(&one, 0, sizeof(one));
        if ((rc = fill_impl(c, metric, as_distance, slab, 0, st, sum ? &one : nullptr))) return rc;
        if (sum) pc_stats_add(*sum, one);
        // test-hooks build only (the release getter answers NULL): the injected triangle stands for the slab as filled
        int64_t hooked_pairs = 0;
        if (const double* const hooked = pc_hooked_slab_values(&hooked_pairs)) {
            if (hooked_pairs != pairs_below(c->dev.N)) {
                pc_set_error("slab walk: pc_hook_slab_values holds %lld values, the triangle of %d genomes has %lld", (long long)hooked_pairs, c->dev.N,
                             (long long)pairs_below(c->dev.N));
                return PC_ERR_ARG;
            }
            PC_HIP(hipMemcpyAsync(slab, hooked + pairs_below(t0), (size_t)Lp * 8, hipMemcpyHostToDevice, st));
        }
        if ((rc = hook(slab, Lp, c->shard))) return rc;
    }
    return PC_OK;
}

// ---- the drivers ----
// The walk of a fill over the targets [ta, tb): the cut, and every slab to the description's slab().
template <class Fill> int pc_slab_stretch(pc_ctx* c, PcSlabRun& run, int ta, int tb) {
    if (!stretch_ok(c, run, ta, tb)) return PC_ERR_ARG;
    if (c->dev.N <= 1 || ta == tb) return PC_OK;
    std::vector<int32_t> cut;
    int rc = slab_cut(c, run.max_pairs, ta, tb, cut);
    if (rc != PC_OK) return rc;
    rc = slab_walk(c, cut, run.metric, run.as_distance, run.timed ? &run.sum : nullptr,
                   [&](const double* slab, int64_t Lp, const PcShard& shard) -> int { return Fill::slab(c, run, slab, Lp, shard); });
    if (rc != PC_OK) return rc;
    run.n_slabs += (int32_t)cut.size() - 1;
    return PC_OK;
}
// A fill on one context.
template <class Fill> int pc_slab_fill(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    if ((rc = pc_slab_check(c, run, Fill::what))) return rc;
    PC_ON_DEVICE(c);
    PcRange range(Fill::range);
    if ((rc = Fill::begin(c, run)) || (rc = pc_slab_stretch<Fill>(c, run, 0, c->dev.N))) return rc;
    return Fill::end(c, run);
}
template int pc_slab_fill<PcEdgesFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_fill<PcComponentsFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_fill<PcNearestFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_fill<PcTreeFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_fill<PcBetweenFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_stretch<PcEdgesFill>(pc_ctx*, PcSlabRun&, int, int);
template int pc_slab_stretch<PcComponentsFill>(pc_ctx*, PcSlabRun&, int, int);
template int pc_slab_stretch<PcNearestFill>(pc_ctx*, PcSlabRun&, int, int);
template int pc_slab_stretch<PcTreeFill>(pc_ctx*, PcSlabRun&, int, int);
template int pc_slab_stretch<PcBetweenFill>(pc_ctx*, PcSlabRun&, int, int);
template int pc_slab_fill<PcAffinityFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_stretch<PcAffinityFill>(pc_ctx*, PcSlabRun&, int, int);
template int pc_slab_fill<PcHistFill>(pc_ctx*, PcSlabRun&);
template int pc_slab_stretch<PcHistFill>(pc_ctx*, PcSlabRun&, int, int);

// ---- what the descriptions share ----
// begin, ahead of anything of the fill's own: the run and the fill's two times (last_ms) reset, the loan of an earlier call ended (its
// buffers are rewritten) ...
static int slab_begin(pc_ctx* c, PcSlabRun& run, float* last_ms) {
    memset(&run.sum, 0, sizeof(run.sum)); run.n_slabs = 0; run.n_edges = 0; run.pending = false;
    last_ms[0] = last_ms[1] = 0.f;
    return wait_last_work(c, c->stream, false);
}
// ... and, N > 1, before the fill allocates anything on the device: the slab size, the events of a timed run
static int slab_size(pc_ctx* c, PcSlabRun& run) {
    run.max_pairs = slab_max_pairs(c, run.slab_bytes, run.rows_form ? (int64_t)run.n_query * c->dev.N : pairs_below(c->dev.N));
    if (run.timed) for (hipEvent_t& e : c->ev_slab) if (!e) PC_HIP(hipEventCreate(&e));
    return PC_OK;
}
// the pending pass's time (events 0 and 1) added to *slot
static int slab_add_pass_time(pc_ctx* c, const PcSlabRun& run, float* slot) {
    if (!run.timed || !run.pending) return PC_OK;
    float x = 0.f;
    PC_HIP(hipEventElapsedTime(&x, c->ev_slab[0], c->ev_slab[1]));
    *slot += x;
    return PC_OK;
}
// A slab's pass of a components / nearest fill, left running (the walk has waited for the pass before it: its two events can be read).
template <class Launch> static int slab_pass(pc_ctx* c, PcSlabRun& run, float* last_ms, Launch launch) {
    int rc = PC_OK;
    hipStream_t st = c->stream;
    if ((rc = slab_add_pass_time(c, run, &last_ms[0]))) return rc;
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[0], st));
    if ((rc = launch(st))) return rc;
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[1], st));
    run.pending = true;
    return mark_work(c, st);
}
// ... and after the last slab: the closing pass, ONE D2H of what it wrote, the stream drained; the last slab's pass and this one timed.
template <class Launch> static int slab_finish(pc_ctx* c, PcSlabRun& run, float* last_ms, void* host, const void* dev, size_t bytes, Launch launch) {
    int rc = PC_OK;
    hipStream_t st = c->stream;
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[2], st));
    if ((rc = launch(st))) return rc;
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[3], st));
    PC_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    if ((rc = slab_add_pass_time(c, run, &last_ms[0]))) return rc;
    if (run.timed) PC_HIP(hipEventElapsedTime(&last_ms[1], c->ev_slab[2], c->ev_slab[3]));
    run.pending = false;
    return PC_OK;
}
static int last_times(const pc_ctx* c, const char* who, const float* last_ms, float* a, float* b) {
    if (!c) { pc_set_error("%s: NULL context", who); return PC_ERR_ARG; }
    if (a) *a = last_ms[0];
    if (b) *b = last_ms[1];
    return PC_OK;
}

// ---- edge-list fill: the pairs whose value passes a threshold, as (source, target, value) arrays sorted by target, then source --
// what matrix_to_adjacency(skip_zero) writes and SymMatrix.nearest_neighbors answers from the dense matrix (matrix.py:536-551,
// 265-296), without the dense matrix ever crossing PCIe.  Each filled slab is compacted (count -> scan -> one 4-byte read-back -> emit,
// pc_edges.hip) and its edges appended to the pinned host result; slabs in ascending target order make the concatenation globally ordered.
int PcEdgesFill::begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    if ((rc = slab_begin(c, run, c->last_edge_ms)) || (rc = c->h_edge_src.ensure(16)) || (rc = c->h_edge_tgt.ensure(16)) || (rc = c->h_edge_val.ensure(16))) return rc;
    if (c->dev.N <= 1) return PC_OK;
    if ((rc = slab_size(c, run))) return rc;
    return run.by_bars ? upload_raw(c->b_edge_bars, run.bars, (size_t)c->dev.N * 8) : (int)PC_OK;     // (resident for the call)
}
// compact: count -> scan (n + 1 elements: the total falls out) -> read the total back -> emit; count(cnt, st) and emit(off, st) launch
// the two passes
template <class Count, class Emit> static int edges_slab(pc_ctx* c, PcSlabRun& run, int64_t Lp, Count count, Emit emit) {
    int rc = PC_OK;
    hipStream_t st = c->stream;
    const bool stats = run.timed;
    uint32_t* const h_total = c->h_plan.as<uint32_t>();
    int64_t& E = run.n_edges;
    const int64_t nch = pc_edge_chunks(Lp);
    if ((rc = c->b_edge_cnt.ensure((size_t)(nch + 1) * 4)) || (rc = c->b_edge_off.ensure((size_t)(nch + 1) * 4)) ||
        (rc = c->b_scan_tmp.ensure((size_t)pc_scan_tmp_elems(nch + 1) * 4))) return abi_rc(rc);
    uint32_t* const cnt = c->b_edge_cnt.as<uint32_t>(); uint32_t* const off = c->b_edge_off.as<uint32_t>();
    if (stats) PC_HIP(hipEventRecord(c->ev_slab[0], st));
    PC_HIP(hipMemsetAsync(cnt + nch, 0, 4, st));
    if ((rc = count(cnt, st))) return rc;
    if ((rc = pc_scan_exclusive_u32(cnt, off, nch + 1, c->b_scan_tmp.as<uint32_t>(), (int64_t)(c->b_scan_tmp.cap / 4), st))) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_slab[1], st));
    PC_HIP(hipMemcpyAsync(h_total, off + nch, 4, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    const int64_t Es = (int64_t)h_total[0];
    if (Es == 0) {
        if (stats) { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, c->ev_slab[0], c->ev_slab[1])); c->last_edge_ms[0] += x; }
        return PC_OK;
    }
    if ((rc = c->b_edge_src.ensure((size_t)Es * 4)) || (rc = c->b_edge_tgt.ensure((size_t)Es * 4)) || (rc = c->b_edge_val.ensure((size_t)Es * 8))) return abi_rc(rc);
    if ((rc = c->h_edge_src.grow_keep((size_t)(E + Es) * 4, (size_t)E * 4)) || (rc = c->h_edge_tgt.grow_keep((size_t)(E + Es) * 4, (size_t)E * 4)) ||
        (rc = c->h_edge_val.grow_keep((size_t)(E + Es) * 8, (size_t)E * 8))) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_slab[2], st));
    if ((rc = emit(off, st))) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_slab[3], st));
    PC_HIP(hipMemcpyAsync(c->h_edge_src.as<int32_t>() + E, c->b_edge_src.p, (size_t)Es * 4, hipMemcpyDeviceToHost, st));
    PC_HIP(hipMemcpyAsync(c->h_edge_tgt.as<int32_t>() + E, c->b_edge_tgt.p, (size_t)Es * 4, hipMemcpyDeviceToHost, st));
    PC_HIP(hipMemcpyAsync(c->h_edge_val.as<double>() + E, c->b_edge_val.p, (size_t)Es * 8, hipMemcpyDeviceToHost, st));
    if (stats) PC_HIP(hipEventRecord(c->ev_slab[4], st));
    PC_HIP(hipStreamSynchronize(st));                                       // the slab, its tables and the edge buffers are rewritten by the next range
    if (stats) {
        float x = 0.f, y = 0.f, z = 0.f;
        PC_HIP(hipEventElapsedTime(&x, c->ev_slab[0], c->ev_slab[1]));
        PC_HIP(hipEventElapsedTime(&y, c->ev_slab[2], c->ev_slab[3]));
        PC_HIP(hipEventElapsedTime(&z, c->ev_slab[3], c->ev_slab[4]));
        c->last_edge_ms[0] += x + y; c->last_edge_ms[1] += z;
    }
    E += Es;
    return PC_OK;
}
int PcEdgesFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    if (run.by_bars) {                                                      // (the triangular walk alone: no rows form takes bars)
        if (dom.is_rows) { pc_set_error("%s: a bar per genome over a rows slab", run.who); return PC_ERR_ARG; }
        const double* const bar = c->b_edge_bars.as<double>();
        return edges_slab(c, run, Lp,
            [&](uint32_t* cnt, hipStream_t st) { return pc_launch_edge_count_bars(slab, Lp, run.as_distance, bar, dom.shard, cnt, st); },
            [&](const uint32_t* off, hipStream_t st) {
                return pc_launch_edge_emit_bars(slab, Lp, run.as_distance, bar, dom.shard, off, c->b_edge_src.as<int32_t>(), c->b_edge_tgt.as<int32_t>(),
                                                c->b_edge_val.as<double>(), st);
            });
    }
    return edges_slab(c, run, Lp,
        [&](uint32_t* cnt, hipStream_t st) { return pc_launch_edge_count(slab, Lp, run.as_distance, run.threshold, dom, cnt, st); },
        [&](const uint32_t* off, hipStream_t st) {
            return pc_launch_edge_emit(slab, Lp, run.as_distance, run.threshold, dom, off, c->b_edge_src.as<int32_t>(), c->b_edge_tgt.as<int32_t>(),
                                       c->b_edge_val.as<double>(), st);
        });
}
// (no end phase of its own on the triangular walk: the edges are in the context's pinned arrays, in order, when a walk returns.  A rows
// slab fill's edges came row-major -- by query row, then by the other genome: one host sort by (target, source), keys distinct)
int PcEdgesFill::end(pc_ctx* c, PcSlabRun& run) {
    int32_t* const src = c->h_edge_src.as<int32_t>(); int32_t* const tgt = c->h_edge_tgt.as<int32_t>(); double* const val = c->h_edge_val.as<double>();
    run.src = src; run.tgt = tgt; run.val = val;
    if (!run.rows_form || run.n_edges < 2) return PC_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t E = (size_t)run.n_edges;
    std::vector<uint64_t> key(E);
    for (size_t e = 0; e < E; ++e) key[e] = ((uint64_t)(uint32_t)tgt[e] << 32) | (uint32_t)src[e];
    if (!std::is_sorted(key.begin(), key.end())) {
        std::vector<size_t> order(E);
        for (size_t e = 0; e < E; ++e) order[e] = e;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key[a] < key[b]; });
        std::vector<double> v(val, val + E);
        for (size_t e = 0; e < E; ++e) { src[e] = (int32_t)(uint32_t)key[order[e]]; tgt[e] = (int32_t)(key[order[e]] >> 32); val[e] = v[order[e]]; }
    }
    if (run.timed) c->last_edge_ms[1] += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PC_OK;
}
// Several devices: nothing travels between them.  The root's pinned arrays are grown to the total and every device's edges laid behind
// those of the ranks before it (ascending stretches: the concatenation is globally ordered); the copy's host time is the exchange.
size_t PcEdgesFill::ship_bytes(const pc_ctx*, const PcSlabRun&) { return 0; }
int PcEdgesFill::ship(pc_ctx*, pc_ctx*, PcSlabRun&, void*, int, int) { return PC_OK; }
int PcEdgesFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void*, int, float* ms_exchange) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    int64_t total = 0;
    for (const PcSlabRun& run : runs) total += run.n_edges;
    const int64_t own = runs[0].n_edges;
    if (total == own) return PC_OK;
    if ((rc = root->h_edge_src.grow_keep((size_t)total * 4, (size_t)own * 4)) || (rc = root->h_edge_tgt.grow_keep((size_t)total * 4, (size_t)own * 4)) ||
        (rc = root->h_edge_val.grow_keep((size_t)total * 8, (size_t)own * 8))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    int64_t at = own;
    for (size_t r = 1; r < ctx.size(); ++r) {
        const int64_t E = runs[r].n_edges;
        if (E == 0) continue;
        memcpy(root->h_edge_src.as<int32_t>() + at, ctx[r]->h_edge_src.p, (size_t)E * 4);
        memcpy(root->h_edge_tgt.as<int32_t>() + at, ctx[r]->h_edge_tgt.p, (size_t)E * 4);
        memcpy(root->h_edge_val.as<double>() + at, ctx[r]->h_edge_val.p, (size_t)E * 8);
        at += E;
    }
    *ms_exchange = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    runs[0].n_edges = total;
    return PC_OK;
}

extern "C" int pc_fill_edges(pc_ctx* c, int metric, int as_distance, double threshold, int64_t slab_bytes,
                             const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_edges"; run.metric = metric; run.as_distance = as_distance; run.threshold = threshold; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcEdgesFill>(run, {src, tgt, val, n_edges, n_slabs}, stats, [&] { return pc_slab_fill<PcEdgesFill>(c, run); });
}

// the same fill with a bar per genome (host memory, f64[N]) in the threshold's place
extern "C" int pc_fill_edges_bars(pc_ctx* c, int metric, int as_distance, const double* bar, int64_t slab_bytes,
                                  const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_edges_bars"; run.metric = metric; run.as_distance = as_distance; run.by_bars = true; run.bars = bar;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcEdgesFill>(run, {src, tgt, val, n_edges, n_slabs}, stats, [&] { return pc_slab_fill<PcEdgesFill>(c, run); });
}

extern "C" int pc_last_edge_times(const pc_ctx* c, float* ms_compact, float* ms_d2h) {
    return last_times(c, "pc_last_edge_times", c ? c->last_edge_ms : nullptr, ms_compact, ms_d2h);
}

// ---- components fill: the connected components of the graph {pairs that pass the threshold} -- with a strict distance predicate the
// reference's single-linkage clusters at that eps (clustering.py:4-51) -- as labels[N], the smallest member's index.  Each filled slab
// goes through ONE pass, k_cc_union (pc_components.hip), over a parent[N] array that stays on the device from the first slab to the
// last; nothing is read back per slab.  After the last slab: k_cc_labels, then one D2H of labels[N] and the 8-byte count of passing
// pairs behind them.
static size_t cc_label_bytes(int N) { return ((size_t)std::max(N, 1) * 4 + 7) / 8 * 8; }   // the 64-bit count sits behind the labels, aligned
static unsigned long long* cc_pass_counter(const pc_ctx* c) { return (unsigned long long*)((char*)c->b_cc_labels.p + cc_label_bytes(c->dev.N)); }

int PcComponentsFill::begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N;
    const size_t label_bytes = cc_label_bytes(N);
    if ((rc = slab_begin(c, run, c->last_cc_ms)) || (rc = c->h_cc_labels.ensure(label_bytes + 8))) return rc;
    if (N <= 1) return PC_OK;
    if ((rc = slab_size(c, run))) return rc;
    if ((rc = c->b_cc_parent.ensure((size_t)N * 4)) || (rc = c->b_cc_labels.ensure(label_bytes + 8))) return abi_rc(rc);
    return pc_launch_cc_init(c->b_cc_parent.as<int32_t>(), N, cc_pass_counter(c), c->stream);
}
int PcComponentsFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    return slab_pass(c, run, c->last_cc_ms, [&](hipStream_t st) {
        return pc_launch_cc_union(slab, Lp, run.as_distance, run.strict, run.threshold, dom, c->b_cc_parent.as<int32_t>(), cc_pass_counter(c), st);
    });
}
// (run.n_edges comes in as the pairs that passed on other devices: a pair lies in exactly one stretch)
int PcComponentsFill::end(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N;
    const size_t label_bytes = cc_label_bytes(N);
    int32_t* const h_labels = c->h_cc_labels.as<int32_t>();
    run.labels = h_labels;
    if (N <= 1) {
        if (N == 1) { h_labels[0] = 0; run.n_components = 1; }
        return PC_OK;
    }
    if ((rc = slab_finish(c, run, c->last_cc_ms, h_labels, c->b_cc_labels.p, label_bytes + 8, [&](hipStream_t st) {
            return pc_launch_cc_labels(c->b_cc_parent.as<int32_t>(), c->b_cc_labels.as<int32_t>(), N, st);
        }))) return rc;
    int32_t comps = 0;
    for (int g = 0; g < N; ++g) comps += h_labels[g] == g;
    unsigned long long passed = 0;
    memcpy(&passed, (const char*)h_labels + label_bytes, 8);
    run.n_components = comps; run.n_edges += (int64_t)passed;
    return PC_OK;
}
// Several devices: a device ships its forest, parent[N], and copies its 8-byte count of passing pairs to the host (into its run); the
// root unites the forests with its own in one launch (k_cc_merge) and takes the counts in.
size_t PcComponentsFill::ship_bytes(const pc_ctx* root, const PcSlabRun&) { return (size_t)root->dev.N * 4; }
int PcComponentsFill::ship(pc_ctx* c, pc_ctx* root, PcSlabRun& run, void* stage, int slot, int) {
    int rc = PC_OK;
    const size_t N = (size_t)c->dev.N;
    PC_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = pc_ship(c, root, (int32_t*)stage + (size_t)slot * N, c->b_cc_parent.p, N * 4))) return rc;
    PC_HIP(hipEventRecord(c->ev[1], c->stream));
    PC_HIP(hipMemcpyAsync(&run.n_edges, cc_pass_counter(c), 8, hipMemcpyDeviceToHost, c->stream));
    return PC_OK;
}
int PcComponentsFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float*) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    for (size_t r = 1; r < runs.size(); ++r) runs[0].n_edges += runs[r].n_edges;
    PC_HIP(hipEventRecord(root->ev[0], root->stream));
    if ((rc = pc_launch_cc_merge(root->b_cc_parent.as<int32_t>(), (const int32_t*)stage, n_foreign, root->dev.N, root->stream))) return rc;
    PC_HIP(hipEventRecord(root->ev[1], root->stream));
    return PC_OK;
}

extern "C" int pc_fill_components(pc_ctx* c, int metric, int as_distance, double threshold, int strict, int64_t slab_bytes,
                                  const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_components"; run.metric = metric; run.as_distance = as_distance; run.strict = strict; run.threshold = threshold;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcComponentsFill>(run, {labels, n_components, n_edges, n_slabs}, stats, [&] { return pc_slab_fill<PcComponentsFill>(c, run); });
}

extern "C" int pc_last_component_times(const pc_ctx* c, float* ms_union, float* ms_labels) {
    return last_times(c, "pc_last_component_times", c ? c->last_cc_ms : nullptr, ms_union, ms_labels);
}

// ---- nearest-neighbours fill: each genome's k best neighbours in the total order (value, better first; then index) -- what
// SymMatrix.nearest_neighbors answers per node from the dense matrix (matrix.py:265-296), cut after k -- as nbr[N][kk], val[N][kk].
// Each filled slab goes through two passes (pc_nearest.hip: k_nn_rows, k_nn_cols) over key[N][kk] / nbr[N][kk], which stay on the
// device from the first slab to the last; nothing is read back per slab.  After the last slab: k_nn_finish, then one D2H of
// val[N][kk] with nbr[N][kk] behind it.
static size_t nn_entries(const pc_ctx* c, const PcSlabRun& run) { return (size_t)std::max(c->dev.N, 0) * run.kk; }
static int32_t* nn_nbr(const pc_ctx* c, const PcSlabRun& run) { return (int32_t*)((char*)c->b_nn_out.p + nn_entries(c, run) * 8); }

int PcNearestFill::begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const size_t n_ent = nn_entries(c, run), out_bytes = n_ent * 8 + n_ent * 4;
    if ((rc = slab_begin(c, run, c->last_nn_ms)) || (rc = c->h_nn.ensure(std::max<size_t>(out_bytes, 16)))) return rc;
    if (c->dev.N <= 1) return PC_OK;
    if ((rc = slab_size(c, run))) return rc;
    if ((rc = c->b_nn_key.ensure(n_ent * 8)) || (rc = c->b_nn_out.ensure(out_bytes))) return abi_rc(rc);
    return pc_launch_nn_init(c->b_nn_key.as<unsigned long long>(), nn_nbr(c, run), (int64_t)n_ent, c->stream);
}
// the row pass, then the column pass: a triangular slab's targets are the consecutive range that starts at its first owned one; a rows
// slab goes through the rows forms of the two passes (k_nn_qrows, k_nn_qcols)
int PcNearestFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    unsigned long long* const key = c->b_nn_key.as<unsigned long long>();
    if (dom.is_rows)
        return slab_pass(c, run, c->last_nn_ms, [&](hipStream_t st) { return pc_launch_nn_select_rows(slab, Lp, dom.rows, run.as_distance, run.kk, key, nn_nbr(c, run), st); });
    const int t0 = c->h_owned[0], t1 = t0 + dom.shard.nown;
    return slab_pass(c, run, c->last_nn_ms, [&](hipStream_t st) {
        return pc_launch_nn_select(slab, Lp, t0, t1, run.as_distance, run.kk, key, nn_nbr(c, run), st);
    });
}
int PcNearestFill::end(pc_ctx* c, PcSlabRun& run) {
    const size_t n_ent = nn_entries(c, run), val_bytes = n_ent * 8, out_bytes = val_bytes + n_ent * 4;
    run.val = c->h_nn.as<double>(); run.nbr = (const int32_t*)((const char*)c->h_nn.p + val_bytes);
    if (c->dev.N <= 1) return PC_OK;
    return slab_finish(c, run, c->last_nn_ms, c->h_nn.p, c->b_nn_out.p, out_bytes, [&](hipStream_t st) {
        return pc_launch_nn_finish(c->b_nn_key.as<unsigned long long>(), c->b_nn_out.as<double>(), (int64_t)n_ent, run.as_distance, st);
    });
}
// Several devices: a device ships its lists in key space -- the staging buffer holds [n_foreign][N][kk] keys, then as many indices --
// and the root merges them into its own by the one total order (k_nn_merge).
size_t PcNearestFill::ship_bytes(const pc_ctx* root, const PcSlabRun& run) { return nn_entries(root, run) * 12; }
int PcNearestFill::ship(pc_ctx* c, pc_ctx* root, PcSlabRun& run, void* stage, int slot, int n_foreign) {
    int rc = PC_OK;
    const size_t n_ent = nn_entries(c, run);
    unsigned long long* const stage_key = (unsigned long long*)stage;
    int32_t* const stage_nbr = (int32_t*)(stage_key + (size_t)n_foreign * n_ent);
    PC_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = pc_ship(c, root, stage_key + (size_t)slot * n_ent, c->b_nn_key.p, n_ent * 8)) ||
        (rc = pc_ship(c, root, stage_nbr + (size_t)slot * n_ent, nn_nbr(c, run), n_ent * 4))) return rc;
    PC_HIP(hipEventRecord(c->ev[1], c->stream));
    return PC_OK;
}
int PcNearestFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float*) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    const unsigned long long* const stage_key = (const unsigned long long*)stage;
    const int32_t* const stage_nbr = (const int32_t*)(stage_key + (size_t)n_foreign * nn_entries(root, runs[0]));
    PC_HIP(hipEventRecord(root->ev[0], root->stream));
    if ((rc = pc_launch_nn_merge(root->b_nn_key.as<unsigned long long>(), nn_nbr(root, runs[0]), stage_key, stage_nbr, n_foreign, root->dev.N, runs[0].kk,
                                 root->stream))) return rc;
    PC_HIP(hipEventRecord(root->ev[1], root->stream));
    return PC_OK;
}

extern "C" int pc_fill_nearest(pc_ctx* c, int metric, int as_distance, int k, int64_t slab_bytes,
                               const int32_t** nbr, const double** val, int32_t* k_out, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_nearest"; run.metric = metric; run.as_distance = as_distance; run.k = k; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcNearestFill>(run, {nbr, val, k_out, n_slabs}, stats, [&] { return pc_slab_fill<PcNearestFill>(c, run); });
}

extern "C" int pc_last_nearest_times(const pc_ctx* c, float* ms_select, float* ms_finish) {
    return last_times(c, "pc_last_nearest_times", c ? c->last_nn_ms : nullptr, ms_select, ms_finish);
}

// ---- k-nearest lists of a pair list: no fill and no walk -- the caller's (src, tgt, val)[L] go up once, every pair becomes two directed
// entries (owner << 32 | other, position), one sort makes an owner's entries a run, and one wave per owner selects (pc_nearest.hip:
// k_nn_pair_entries, k_nn_run_starts, k_nn_pairs), then k_nn_finish and ONE D2H of val[N][kk] | nbr[N][kk] | count[N] into h_nn.  The
// context gives N and the buffers; neither the sets nor the residues are read.
#define PC_NEAREST_PAIRS_MAX ((int64_t)1 << 30)

extern "C" int pc_nearest_of_pairs(pc_ctx* c, const int32_t* src, const int32_t* tgt, const double* val, int64_t n_pairs, int as_distance, int k,
                                   const int32_t** nbr, const double** val_out, const int32_t** count, int32_t* k_out) {
    const char* const who = "pc_nearest_of_pairs";
    if (nbr) *nbr = nullptr; if (val_out) *val_out = nullptr; if (count) *count = nullptr; if (k_out) *k_out = 0;
    if (!c || !c->uploaded) { pc_set_error("%s: upload first", who); return PC_ERR_STATE; }
    if (k < 1) { pc_set_error("%s: k %d", who, k); return PC_ERR_ARG; }
    if (k > PC_NEAREST_MAX_K) { pc_set_error("%s: k %d is above PC_NEAREST_MAX_K = %d", who, k, PC_NEAREST_MAX_K); return PC_ERR_LIMIT; }
    if (!nbr || !val_out || !count || !k_out) { pc_set_error("%s: an output pointer is NULL", who); return PC_ERR_ARG; }
    if (n_pairs < 0) { pc_set_error("%s: n_pairs %lld", who, (long long)n_pairs); return PC_ERR_ARG; }
    if (n_pairs > PC_NEAREST_PAIRS_MAX) {
        pc_set_error("%s: %lld pairs exceed the 2^30 one call takes (its 2 n_pairs directed entries are sorted with 32-bit values)", who, (long long)n_pairs);
        return PC_ERR_LIMIT;
    }
    if (n_pairs > 0 && (!src || !tgt || !val)) { pc_set_error("%s: %s is NULL", who, !src ? "src" : !tgt ? "tgt" : "val"); return PC_ERR_ARG; }
    const int N = c->dev.N;
    const int64_t L = n_pairs;
    for (int64_t e = 0; e < L; ++e) {
        if (src[e] < 0 || src[e] >= N || tgt[e] < 0 || tgt[e] >= N) {
            pc_set_error("%s: entry %lld is (%d, %d); genome indices lie in [0, %d)", who, (long long)e, src[e], tgt[e], N); return PC_ERR_ARG;
        }
        if (src[e] == tgt[e]) { pc_set_error("%s: entry %lld is the diagonal (%d, %d): a genome is no neighbour of itself", who, (long long)e, src[e], tgt[e]); return PC_ERR_ARG; }
    }
    int rc = PC_OK;
    PC_ON_DEVICE(c);
    PcRange range("pc:nearest_of_pairs");
    hipStream_t st = c->stream;
    const int kk = std::max(std::min(k, N - 1), 0);
    const size_t n_ent = (size_t)std::max(N, 0) * kk, val_bytes = n_ent * 8, out_bytes = val_bytes + n_ent * 4 + (size_t)std::max(N, 0) * 4;
    if ((rc = wait_last_work(c, st, false)) || (rc = c->h_nn.ensure(std::max<size_t>(out_bytes, 16)))) return rc;
    *val_out = c->h_nn.as<double>(); *nbr = (const int32_t*)((const char*)c->h_nn.p + val_bytes); *count = *nbr + n_ent; *k_out = kk;
    if (N < 1) return PC_OK;
    int32_t* const h_count = (int32_t*)((char*)c->h_nn.p + val_bytes + n_ent * 4);
    if (kk == 0) { h_count[0] = 0; return PC_OK; }                         // (N == 1: no pair can be listed)
    int key_bits = 33;
    while (key_bits < 64 && ((int64_t)1 << (key_bits - 32)) < N) ++key_bits;
    rc = [&]() -> int {
        int rc = PC_OK;
        if ((rc = c->b_nn_key.ensure(n_ent * 8)) || (rc = c->b_nn_out.ensure(out_bytes)) || (rc = c->b_np_start.ensure((size_t)(N + 1) * 4)) ||
            (rc = c->b_key0.ensure(std::max<size_t>((size_t)L * 16, 16))) || (rc = c->b_key1.ensure(std::max<size_t>((size_t)L * 16, 16))) ||
            (rc = c->b_val0.ensure(std::max<size_t>((size_t)L * 8, 16))) || (rc = c->b_val1.ensure(std::max<size_t>((size_t)L * 8, 16))) ||
            (rc = c->b_sort_tmp.ensure(std::max<size_t>(pc_sort_temp_bytes(2 * L, key_bits), 16)))) return abi_rc(rc);
        if ((rc = upload_raw(c->b_pr_src, src, (size_t)L * 4)) || (rc = upload_raw(c->b_pr_tgt, tgt, (size_t)L * 4)) ||
            (rc = upload_raw(c->b_np_val, val, (size_t)L * 8))) return rc;
        unsigned long long* const key = c->b_nn_key.as<unsigned long long>();
        double* const d_val = c->b_nn_out.as<double>();
        int32_t* const d_nbr = (int32_t*)((char*)c->b_nn_out.p + val_bytes); int32_t* const d_count = d_nbr + n_ent;
        if ((rc = pc_launch_nn_pair_entries(c->b_pr_src.as<int32_t>(), c->b_pr_tgt.as<int32_t>(), c->b_key0.as<unsigned long long>(), c->b_val0.as<uint32_t>(), L, st)) ||
            (rc = pc_sort_pairs(c->b_sort_tmp.p, c->b_sort_tmp.cap, c->b_key0.as<unsigned long long>(), c->b_key1.as<unsigned long long>(),
                                c->b_val0.as<uint32_t>(), c->b_val1.as<uint32_t>(), 2 * L, key_bits, st)) ||
            (rc = pc_launch_nn_of_pairs(c->b_key1.as<unsigned long long>(), c->b_val1.as<uint32_t>(), c->b_np_val.as<double>(), L, N, as_distance ? 1 : 0, kk,
                                        c->b_np_start.as<uint32_t>(), key, d_nbr, d_count, st)) ||
            (rc = pc_launch_nn_finish(key, d_val, (int64_t)n_ent, as_distance ? 1 : 0, st))) return rc;
        PC_HIP(hipMemcpyAsync(c->h_nn.p, c->b_nn_out.p, out_bytes, hipMemcpyDeviceToHost, st));
        PC_HIP(hipStreamSynchronize(st));
        c->busy = false;
        return PC_OK;
    }();
    if (rc != PC_OK) {
        (void)hipStreamSynchronize(st);                                     // (nothing of a refused call stays in flight over the buffers)
        *nbr = nullptr; *val_out = nullptr; *count = nullptr; *k_out = 0;
    }
    return rc;
}

// ---- tree fill: the single-linkage dendrogram as the N - 1 edges of the minimum spanning tree under the one total order (value, better
// first; then t; then s), delivered in that order -- the merge order.  Each filled slab goes through one PASS of Boruvka rounds
// (pc_tree.hip) over the resident forest and the slab, into the context's second list; then the lists swap.  The forest, a list of keys
// with its counters behind them, stays on the device from the first slab to the last; nothing is read back per slab.  After the last
// slab: one D2H of the list, then the host sorts the keys and decodes them into the pinned result.
static size_t tree_list_words(const pc_ctx* c) { return (size_t)std::max(c->dev.N, 1) + PC_TREE_TAIL; }
static unsigned long long* tree_list(const pc_ctx* c, int which) { return c->b_tree_list.as<unsigned long long>() + (size_t)which * tree_list_words(c); }

int PcTreeFill::begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N;
    const size_t words = tree_list_words(c);
    run.tree_launched = 0;
    c->last_tree_rounds[0] = c->last_tree_rounds[1] = 0; c->tree_cur = 0;
    if ((rc = slab_begin(c, run, c->last_tree_ms)) || (rc = c->h_tree.ensure((size_t)std::max(N, 1) * 16)) || (rc = c->h_tree_keys.ensure(words * 8))) return rc;
    if (N <= 1) return PC_OK;
    if ((rc = slab_size(c, run))) return rc;
    if ((rc = c->b_tree_comp.ensure((size_t)N * 8)) || (rc = c->b_tree_best.ensure((size_t)N * 8)) || (rc = c->b_tree_list.ensure(words * 16)) ||
        (rc = c->b_tree_live.ensure(((size_t)pc_tree_round_count(N) + 1) * 4))) return abi_rc(rc);
    PC_HIP(hipMemsetAsync(tree_list(c, 0) + (N - 1), 0, 24, c->stream));       // the empty forest: no key, no violation, no round
    return PC_OK;
}
// One pass: the resident forest, the slab with its pair domain (dom != NULL) and n_foreign staged lists into the other list, which becomes
// the resident one.
static int tree_pass(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain* dom, const unsigned long long* foreign,
                     int n_foreign, hipStream_t st) {
    int rc = PC_OK;
    const int N = c->dev.N, rounds = pc_tree_round_count(N);
    const size_t words = tree_list_words(c);
    int32_t* const comp = c->b_tree_comp.as<int32_t>(); int32_t* const next = comp + N;
    unsigned long long* const best = c->b_tree_best.as<unsigned long long>();
    uint32_t* const live = c->b_tree_live.as<uint32_t>();
    const unsigned long long* const kept = tree_list(c, c->tree_cur);
    unsigned long long* const out = tree_list(c, c->tree_cur ^ 1);
    if ((rc = pc_launch_tree_reset(comp, best, live, rounds, kept, out, N, st)) || (rc = pc_launch_tree_take_counts(out, foreign, n_foreign, N, st))) return rc;
    for (int r = 0; r < rounds; ++r) {
        if (dom && (rc = pc_launch_tree_scan_slab(slab, Lp, run.as_distance, *dom, comp, best, out, N, live, r, st))) return rc;
        if ((rc = pc_launch_tree_scan_list(kept, comp, best, N, live, r, st))) return rc;
        for (int f = 0; f < n_foreign; ++f) if ((rc = pc_launch_tree_scan_list(foreign + (size_t)f * words, comp, best, N, live, r, st))) return rc;
        if ((rc = pc_launch_tree_hook(comp, next, best, out, N, live, r, st)) || (rc = pc_launch_tree_flatten(comp, next, best, out, N, live, r, st))) return rc;
    }
    c->tree_cur ^= 1;
    run.tree_launched += rounds;
    return PC_OK;
}
int PcTreeFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    return slab_pass(c, run, c->last_tree_ms, [&](hipStream_t st) { return tree_pass(c, run, slab, Lp, &dom, nullptr, 0, st); });
}
int PcTreeFill::end(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N;
    double* const val = c->h_tree.as<double>();
    int32_t* const src = (int32_t*)(val + std::max(N, 1)); int32_t* const tgt = src + std::max(N, 1);
    run.val = val; run.src = src; run.tgt = tgt; run.n_edges = 0;
    if (N <= 1) return PC_OK;
    hipStream_t st = c->stream;
    PC_HIP(hipStreamSynchronize(st));                                       // (the last pass's rounds: not part of the finish)
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long* const keys = c->h_tree_keys.as<unsigned long long>();
    PC_HIP(hipMemcpyAsync(keys, tree_list(c, c->tree_cur), tree_list_words(c) * 8, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    if ((rc = slab_add_pass_time(c, run, &c->last_tree_ms[0]))) return rc;
    run.pending = false;
    const unsigned long long count = keys[N - 1], bad = keys[N];
    c->last_tree_rounds[0] = (int32_t)keys[N + 1]; c->last_tree_rounds[1] = run.tree_launched;
    if (bad) {
        pc_set_error("%s: %llu values of the fill are no millionth in [0, 1]: the order of the tree is not defined on them", run.who, bad);
        return PC_ERR_DATA;
    }
    if (count != (unsigned long long)(N - 1)) { pc_set_error("%s: the forest holds %llu edges, not %d", run.who, count, N - 1); return PC_ERR_HIP; }
    std::sort(keys, keys + count);
    for (int i = 0; i < N - 1; ++i) {
        const int micro = pc_tree_key_micro(keys[i]), s = pc_tree_key_s(keys[i]), t = pc_tree_key_t(keys[i]);
        if (micro > PC_TREE_MICRO_MAX || s >= t || t >= N) { pc_set_error("%s: edge %d of the forest is no key (%llx)", run.who, i, keys[i]); return PC_ERR_HIP; }
        src[i] = s; tgt[i] = t;
        val[i] = (double)(run.as_distance ? micro : PC_TREE_MICRO_MAX - micro) / 1000000.0;
    }
    run.n_edges = N - 1;
    c->last_tree_ms[1] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return PC_OK;
}
// Several devices: a device ships its forest -- the list, its counters behind the keys -- and the root runs one pass over its own
// forest and the staged ones (lists only), which takes their counters in; the rounds the devices enqueued are summed on the host.
size_t PcTreeFill::ship_bytes(const pc_ctx* root, const PcSlabRun&) { return tree_list_words(root) * 8; }
int PcTreeFill::ship(pc_ctx* c, pc_ctx* root, PcSlabRun&, void* stage, int slot, int) {
    int rc = PC_OK;
    const size_t words = tree_list_words(c);
    PC_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = pc_ship(c, root, (unsigned long long*)stage + (size_t)slot * words, tree_list(c, c->tree_cur), words * 8))) return rc;
    PC_HIP(hipEventRecord(c->ev[1], c->stream));
    return PC_OK;
}
int PcTreeFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float*) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    for (size_t r = 1; r < runs.size(); ++r) runs[0].tree_launched += runs[r].tree_launched;
    PC_HIP(hipEventRecord(root->ev[0], root->stream));
    if (n_foreign > 0 && (rc = tree_pass(root, runs[0], nullptr, 0, nullptr, (const unsigned long long*)stage, n_foreign, root->stream))) return rc;
    PC_HIP(hipEventRecord(root->ev[1], root->stream));
    return PC_OK;
}

extern "C" int pc_fill_tree(pc_ctx* c, int metric, int as_distance, int64_t slab_bytes,
                            const int32_t** src, const int32_t** tgt, const double** val, int32_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_tree"; run.metric = metric; run.as_distance = as_distance; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcTreeFill>(run, {src, tgt, val, n_edges, n_slabs}, stats, [&] { return pc_slab_fill<PcTreeFill>(c, run); });
}

extern "C" int pc_last_tree_times(const pc_ctx* c, float* ms_rounds, float* ms_finish) {
    return last_times(c, "pc_last_tree_times", c ? c->last_tree_ms : nullptr, ms_rounds, ms_finish);
}

extern "C" int pc_last_tree_rounds(const pc_ctx* c, int32_t* live_rounds, int32_t* launched_rounds) {
    if (!c) { pc_set_error("pc_last_tree_rounds: NULL context"); return PC_ERR_ARG; }
    if (live_rounds) *live_rounds = c->last_tree_rounds[0];
    if (launched_rounds) *launched_rounds = c->last_tree_rounds[1];
    return PC_OK;
}

// ---- between-groups fill: for a partition of the genomes into G groups the G x G table of the count, sum, minimum and maximum of the
// pair values between every two groups, in millionths -- what the reference's dataset heatmap in cluster order shows (matrix.py,
// scripts/phamclust.py:433) and what single, complete and average linkage between clusters are.  Each filled slab goes through ONE pass,
// k_between_rows (pc_between.hip), over an accumulator that stays on the device from the first slab to the last; nothing is read back
// per slab.  After the last slab: k_between_fold, then one D2H of the four arrays and the 8-byte violation count behind them.  The walk
// always fills distances (the entry points set as_distance = 1 and keep what the caller asked for in bt_invert): a similarity table is
// the distance table inverted by the fold, as SymMatrix.invert() inverts a matrix.  The rows form, pc_fill_rows_between, seeds the accumulator
// with a stored table (PcBetweenSeed, with the seeds below) and passes the new genomes' rows through k_between_qrows: begin and end are these.
int PcBetweenFill::begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N, G = run.n_groups;
    const size_t bytes = pc_between_bytes(G);
    if ((rc = slab_begin(c, run, c->last_bt_ms)) || (rc = c->h_bt.ensure(bytes))) return rc;
    if (N <= 1) return PC_OK;
    if ((rc = slab_size(c, run))) return rc;
    if ((rc = c->b_bt_acc.ensure(bytes)) || (rc = c->b_bt_out.ensure(bytes))) return abi_rc(rc);
    if ((rc = upload_raw(c->b_bt_group, run.group, (size_t)N * 4))) return rc;
    return pc_launch_between_init(c->b_bt_acc.p, G, c->stream);
}
// A rows slab (pc_fill_rows_between) goes through the rows form of the pass, k_between_qrows, into the same accumulator.
int PcBetweenFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    if (dom.is_rows != run.rows_form) { pc_set_error("%s: a slab of the other pair domain", run.who); return PC_ERR_ARG; }
    if (dom.is_rows)
        return slab_pass(c, run, c->last_bt_ms, [&](hipStream_t st) {
            return pc_launch_between_qrows(slab, Lp, dom.rows, c->b_bt_group.as<int32_t>(), run.n_groups, c->b_bt_acc.p, st);
        });
    const int64_t max_row = c->h_owned.empty() ? 0 : (int64_t)c->h_owned.back();      // (ascending targets, row t holds t values)
    return slab_pass(c, run, c->last_bt_ms, [&](hipStream_t st) {
        return pc_launch_between_rows(slab, Lp, dom.shard, max_row, c->b_bt_group.as<int32_t>(), run.n_groups, c->b_bt_acc.p, st);
    });
}
int PcBetweenFill::end(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int G = run.n_groups;
    const size_t gg = (size_t)G * (size_t)G;
    const PcBetweenAcc h = pc_between_view(c->h_bt.p, G);
    run.bt_sum = (const int64_t*)h.sum; run.bt_cnt = (const int64_t*)h.cnt; run.bt_lo = (const int32_t*)h.lo; run.bt_hi = (const int32_t*)h.hi;
    if (c->dev.N <= 1) {                                                    // no pair: every entry empty
        memset(h.sum, 0, gg * 16);
        for (size_t i = 0; i < gg; ++i) { ((int32_t*)h.lo)[i] = INT32_MAX; ((int32_t*)h.hi)[i] = -1; }
        return PC_OK;
    }
    if ((rc = slab_finish(c, run, c->last_bt_ms, c->h_bt.p, c->b_bt_out.p, pc_between_bytes(G), [&](hipStream_t st) {
            return pc_launch_between_fold(c->b_bt_acc.p, c->b_bt_out.p, G, run.bt_invert, st);
        }))) return rc;
    if (*h.bad) {
        pc_set_error("%s: %llu values of the fill are no millionth in [0, 1]: the table is not defined on them", run.who, *h.bad);
        return PC_ERR_DATA;
    }
    return PC_OK;
}
// Several devices: a device ships its raw accumulator, 24 G^2 + 8 bytes, and the root adds the staged ones into its own in one launch
// (k_between_merge) before it folds: a pair lies in exactly one stretch, so nothing is counted twice.
size_t PcBetweenFill::ship_bytes(const pc_ctx*, const PcSlabRun& run) { return pc_between_bytes(run.n_groups); }
int PcBetweenFill::ship(pc_ctx* c, pc_ctx* root, PcSlabRun& run, void* stage, int slot, int) {
    int rc = PC_OK;
    const size_t bytes = pc_between_bytes(run.n_groups);
    PC_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = pc_ship(c, root, (char*)stage + (size_t)slot * bytes, c->b_bt_acc.p, bytes))) return rc;
    PC_HIP(hipEventRecord(c->ev[1], c->stream));
    return PC_OK;
}
int PcBetweenFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float*) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    PC_HIP(hipEventRecord(root->ev[0], root->stream));
    if ((rc = pc_launch_between_merge(root->b_bt_acc.p, stage, n_foreign, runs[0].n_groups, root->stream))) return rc;
    PC_HIP(hipEventRecord(root->ev[1], root->stream));
    return PC_OK;
}

extern "C" int pc_fill_between(pc_ctx* c, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                               const int64_t** sum, const int64_t** count, const int32_t** lo, const int32_t** hi, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_between"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcBetweenFill>(run, {sum, count, lo, hi, n_slabs}, stats, [&] { return pc_slab_fill<PcBetweenFill>(c, run); });
}

extern "C" int pc_last_between_times(const pc_ctx* c, float* ms_reduce, float* ms_finish) {
    return last_times(c, "pc_last_between_times", c ? c->last_bt_ms : nullptr, ms_reduce, ms_finish);
}
extern "C" int pc_between_max_groups(void) { return PC_BETWEEN_MAX_GROUPS; }
extern "C" int pc_between_segment(void) { return PC_BETWEEN_SEGMENT; }

// ---- affinity fill: for a partition of the genomes into G groups the N x G table of the sum, minimum and maximum of the pair values
// between every genome and every group, in millionths -- the column a medoid is read from (SymMatrix.medoid, matrix.py:80-104, over a
// group's own column), the two entries a silhouette is made of, and the group a genome is nearest to by average, single or complete
// linkage.  Each filled slab goes through TWO passes, k_aff_rows and k_aff_cols (pc_affinity.hip), over a table that stays on the
// device from the first slab to the last; nothing is read back per slab.  After the last slab: k_aff_finish, then one D2H of the O(N)
// arrays (and of the whole table only when the caller asked for it).  The walk always fills distances, as the between-groups fill's.
// What the table may take of the device: half of the HBM that is free when the call begins (the fill's own grow-only buffers counted as
// free); the automatic slab size is read after the table is in place.
extern "C" int pc_affinity_block(void) { return PC_AFFINITY_BLOCK; }
extern "C" int64_t pc_affinity_bytes(int64_t n, int64_t n_groups) {
    if (n < 0 || n_groups < 0 || (n && n_groups > (INT64_MAX - 8) / 16 / n)) return -1;
    return n * n_groups * 16 + 8;
}
// the column pass's group ranges: about `want` of them, cut where the running member count passes equal shares (no range empty)
static void affinity_ranges(const std::vector<int32_t>& goff, int G, int N, int want, std::vector<int32_t>& bounds) {
    const int R = std::max(1, std::min(G, want));
    bounds.assign(1, 0);
    for (int r = 1; r < R; ++r) {
        const int64_t share = (int64_t)N * r / R;
        int a = (int)(std::lower_bound(goff.begin(), goff.begin() + G, (int32_t)share) - goff.begin());
        a = std::max(a, bounds.back() + 1);
        if (a >= G) break;
        bounds.push_back(a);
    }
    bounds.push_back(G);
}
// (test hook, host arithmetic: that cut for a caller's goff[G + 1], goff[0] = 0 ascending to N)
extern "C" int pc_affinity_ranges(const int32_t* goff, int G, int N, int want, int32_t* bounds_out, int cap) {
    if (!goff || G < 1 || N < 0 || cap < 0 || (cap > 0 && !bounds_out)) { pc_set_error("pc_affinity_ranges: bad argument"); return PC_ERR_ARG; }
    if (goff[0] != 0 || goff[G] != N) { pc_set_error("pc_affinity_ranges: goff runs from %d to %d, not from 0 to %d", goff[0], goff[G], N); return PC_ERR_ARG; }
    for (int b = 0; b < G; ++b)
        if (goff[b + 1] < goff[b]) { pc_set_error("pc_affinity_ranges: goff descends at group %d", b); return PC_ERR_ARG; }
    std::vector<int32_t> bounds;
    affinity_ranges(std::vector<int32_t>(goff, goff + G + 1), G, N, want, bounds);
    if (cap > 0 && (size_t)cap < bounds.size()) { pc_set_error("pc_affinity_ranges: %zu bounds, room for %d", bounds.size(), cap); return PC_ERR_ARG; }
    if (cap > 0) memcpy(bounds_out, bounds.data(), bounds.size() * 4);
    return (int)bounds.size() - 1;
}
// The rows form's begin: the state is n_query x G entries and the gain's N (pc_affinity_rows_state_bytes), goff counts the LABELLED genomes
// of each group (queries included: the count of entry [k][b] is size[b] - [group[rows[k]] == b]), qcount the query genomes among them
// (the count of a gain entry).  No query row, or N <= 1: nothing on the device.
static int affinity_rows_begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N, G = run.n_groups, nq = run.n_query, want = run.want_table ? 1 : 0, gain = run.want_gain ? 1 : 0;
    const size_t out_bytes = std::max<size_t>(pc_affinity_rows_out_bytes(nq, std::max(N, 0), G, want, gain), 16);
    c->last_af_ms[2] = 0.f;
    if ((rc = slab_begin(c, run, c->last_af_ms))) return rc;
    if (N <= 1 || nq == 0) return c->h_af.ensure(out_bytes);
    const size_t state_bytes = pc_affinity_rows_state_bytes(nq, N, G), need = state_bytes + (want ? out_bytes : 0);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
    const size_t may = (free_b + c->b_af_tab.cap + c->b_af_out.cap) / 2;
    if (need > may) {
        pc_set_error("%s: the table of %d query rows x %d groups and the gain of %d genomes take %zu bytes on the device (16 n_rows n_groups + 16 N + 8%s), above the %zu they may take (half of the free HBM)",
                     run.who, nq, G, N, need, want ? " and the table's copy for want_table" : "", may);
        return PC_ERR_LIMIT;
    }
    if ((rc = c->h_af.ensure(out_bytes))) return rc;
    if ((rc = c->b_af_tab.ensure(state_bytes)) || (rc = c->b_af_out.ensure(out_bytes))) return abi_rc(rc);
    if ((rc = slab_size(c, run))) return rc;
    std::vector<int32_t> goff((size_t)G + 1, 0), qcount((size_t)G, 0);
    for (int g = 0; g < N; ++g) if (run.group[g] >= 0) ++goff[(size_t)run.group[g] + 1];
    for (int b = 0; b < G; ++b) goff[(size_t)b + 1] += goff[b];
    for (int k = 0; k < nq; ++k) if (run.group[run.query[k]] >= 0) ++qcount[run.group[run.query[k]]];
    if ((rc = upload_raw(c->b_af_group, run.group, (size_t)N * 4)) || (rc = upload_vec(c->b_af_goff, goff)) || (rc = upload_vec(c->b_af_qcount, qcount))) return rc;
    return pc_launch_affinity_rows_init(c->b_af_tab.p, nq, N, G, c->stream);
}
int PcAffinityFill::begin(pc_ctx* c, PcSlabRun& run) {
    if (run.rows_form) return affinity_rows_begin(c, run);
    int rc = PC_OK;
    const int N = c->dev.N, G = run.n_groups, want = run.want_table ? 1 : 0;
    const size_t out_bytes = pc_affinity_out_bytes(std::max(N, 1), G, want);
    c->last_af_ms[2] = 0.f;
    if ((rc = slab_begin(c, run, c->last_af_ms))) return rc;
    if (N <= 1) return c->h_af.ensure(out_bytes);
    const size_t tab_bytes = pc_affinity_table_bytes(N, G), need = tab_bytes + (want ? out_bytes : 0);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
    const size_t may = (free_b + c->b_af_tab.cap + c->b_af_out.cap) / 2;
    if (need > may) {
        pc_set_error("%s: the table of %d genomes x %d groups takes %zu bytes on the device (pc_affinity_bytes%s), above the %zu it may take (half of the free HBM)",
                     run.who, N, G, need, want ? " and its copy for want_table" : "", may);
        return PC_ERR_LIMIT;
    }
    if ((rc = c->h_af.ensure(out_bytes))) return rc;
    if ((rc = c->b_af_tab.ensure(tab_bytes)) || (rc = c->b_af_out.ensure(out_bytes))) return abi_rc(rc);
    if ((rc = slab_size(c, run))) return rc;
    // member: the genomes sorted by (group, index); goff: each group's run
    std::vector<int32_t> goff((size_t)G + 1, 0), member((size_t)N), bounds;
    for (int g = 0; g < N; ++g) ++goff[(size_t)run.group[g] + 1];
    for (int b = 0; b < G; ++b) goff[(size_t)b + 1] += goff[b];
    { std::vector<int32_t> at(goff.begin(), goff.end() - 1); for (int g = 0; g < N; ++g) member[(size_t)at[run.group[g]]++] = g; }
    const int blocks = (N + PC_AFFINITY_BLOCK - 1) / PC_AFFINITY_BLOCK;
    affinity_ranges(goff, G, N, (16 * c->n_cu + blocks - 1) / blocks, bounds);      // about sixteen waves per compute unit over the whole grid
    c->af_ranges = (int)bounds.size() - 1;
    if ((rc = upload_raw(c->b_af_group, run.group, (size_t)N * 4)) || (rc = upload_vec(c->b_af_member, member)) || (rc = upload_vec(c->b_af_goff, goff)) ||
        (rc = upload_vec(c->b_af_range, bounds))) return rc;
    return pc_launch_affinity_init(c->b_af_tab.p, N, G, c->stream);
}
// the two passes' times of the pending slab: events 0, 1 and 4
static int affinity_add_pass_times(pc_ctx* c, const PcSlabRun& run) {
    if (!run.timed || !run.pending) return PC_OK;
    float x = 0.f, y = 0.f;
    PC_HIP(hipEventElapsedTime(&x, c->ev_slab[0], c->ev_slab[1]));
    PC_HIP(hipEventElapsedTime(&y, c->ev_slab[1], c->ev_slab[4]));
    c->last_af_ms[0] += x; c->last_af_ms[2] += y;
    return PC_OK;
}
// A rows slab (pc_fill_rows_affinity) goes through the rows form's two passes: k_aff_qrows, and with want_gain k_aff_qcols.
int PcAffinityFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    if (dom.is_rows != run.rows_form) { pc_set_error("%s: a slab of the other pair domain", run.who); return PC_ERR_ARG; }
    if (dom.is_rows) {
        int rc = PC_OK;
        hipStream_t st = c->stream;
        const int r0 = (int)(dom.rows.rows - c->b_rq_rows.as<int32_t>());     // (the rows walk hands the slab's stretch of the call's rows)
        if ((rc = affinity_add_pass_times(c, run))) return rc;
        if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[0], st));
        if ((rc = pc_launch_affinity_rows_slab(slab, Lp, dom.rows, r0, run.n_query, c->b_af_group.as<int32_t>(), run.n_groups, c->b_af_tab.p, run.want_gain,
                                               run.timed ? c->ev_slab[1] : nullptr, st))) return rc;
        if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[4], st));
        run.pending = true;
        return mark_work(c, st);
    }
    if (c->h_owned.empty() || c->h_owned.back() - c->h_owned.front() + 1 != dom.shard.nown) { pc_set_error("%s: a slab of targets that are not consecutive", run.who); return PC_ERR_ARG; }
    int rc = PC_OK;
    hipStream_t st = c->stream;
    const int N = c->dev.N, G = run.n_groups, t0 = c->h_owned.front();
    if ((rc = affinity_add_pass_times(c, run))) return rc;                  // (the walk has waited for the slab before: its events can be read)
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[0], st));
    if ((rc = pc_launch_affinity_rows(slab, Lp, dom.shard, t0, N, c->b_af_group.as<int32_t>(), G, c->b_af_tab.p, st))) return rc;
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[1], st));
    if ((rc = pc_launch_affinity_cols(slab, Lp, dom.shard, t0, N, c->b_af_member.as<int32_t>(), c->b_af_goff.as<int32_t>(), c->b_af_range.as<int32_t>(),
                                      c->af_ranges, G, c->b_af_tab.p, st))) return rc;
    if (run.timed) PC_HIP(hipEventRecord(c->ev_slab[4], st));
    run.pending = true;
    return mark_work(c, st);
}
// The rows form's end: k_aff_qfinish, ONE D2H of the per-query arrays (and the table, and the gain, where asked for).
static int affinity_rows_end(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = std::max(c->dev.N, 0), G = run.n_groups, nq = run.n_query, want = run.want_table ? 1 : 0, gain = run.want_gain ? 1 : 0;
    const PcAffinityOut h = pc_affinity_out_view(c->h_af.p, nq, G, want);
    const PcAffinityGainOut hg = pc_affinity_gain_view(c->h_af.p, nq, N, G, want, gain);
    run.af_own_sum = (const int64_t*)h.own_sum; run.af_own_lo = h.own_lo; run.af_own_hi = h.own_hi; run.af_near_group = h.near_group;
    run.af_near_sum = (const int64_t*)h.near_sum; run.af_near_lo = h.near_lo; run.af_near_hi = h.near_hi;
    run.af_tab_sum = (const int64_t*)h.tab_sum; run.af_tab_lo = h.tab_lo; run.af_tab_hi = h.tab_hi;
    run.af_gain_sum = (const int64_t*)hg.sum; run.af_gain_lo = hg.lo; run.af_gain_hi = hg.hi;
    if (N <= 1 || nq == 0) {                                                // no pair of the call: every entry empty, no group near
        for (int k = 0; k < nq; ++k) {
            h.own_sum[k] = h.near_sum[k] = 0; h.own_lo[k] = h.near_lo[k] = INT32_MAX; h.own_hi[k] = h.near_hi[k] = -1;
            for (int i = 0; i < 3; ++i) h.near_group[(size_t)i * nq + k] = -1;
            for (int b = 0; want && b < G; ++b) { h.tab_sum[(size_t)k * G + b] = 0; h.tab_lo[(size_t)k * G + b] = INT32_MAX; h.tab_hi[(size_t)k * G + b] = -1; }
        }
        for (int g = 0; gain && g < N; ++g) { hg.sum[g] = 0; hg.lo[g] = INT32_MAX; hg.hi[g] = -1; }
        return PC_OK;
    }
    const bool cols_pending = run.timed && run.pending;
    if ((rc = slab_finish(c, run, c->last_af_ms, c->h_af.p, c->b_af_out.p, pc_affinity_rows_out_bytes(nq, N, G, want, gain), [&](hipStream_t st) {
            return pc_launch_affinity_rows_finish(c->b_af_tab.p, c->b_rq_rows.as<int32_t>(), c->b_af_group.as<int32_t>(), c->b_af_goff.as<int32_t>(),
                                                  c->b_af_qcount.as<int32_t>(), nq, N, G, run.bt_invert, c->b_af_out.p, want, gain, st);
        }))) return rc;
    if (cols_pending) { float y = 0.f; PC_HIP(hipEventElapsedTime(&y, c->ev_slab[1], c->ev_slab[4])); c->last_af_ms[2] += y; }
    if (*h.bad) {
        pc_set_error("%s: %llu pairs of the call hold values that are no millionth in [0, 1]: the table is not defined on them", run.who, *h.bad);
        return PC_ERR_DATA;
    }
    return PC_OK;
}
int PcAffinityFill::end(pc_ctx* c, PcSlabRun& run) {
    if (run.rows_form) return affinity_rows_end(c, run);
    int rc = PC_OK;
    const int N = c->dev.N, G = run.n_groups, want = run.want_table ? 1 : 0;
    const PcAffinityOut h = pc_affinity_out_view(c->h_af.p, std::max(N, 1), G, want);
    run.af_own_sum = (const int64_t*)h.own_sum; run.af_own_lo = h.own_lo; run.af_own_hi = h.own_hi; run.af_near_group = h.near_group;
    run.af_near_sum = (const int64_t*)h.near_sum; run.af_near_lo = h.near_lo; run.af_near_hi = h.near_hi;
    run.af_tab_sum = (const int64_t*)h.tab_sum; run.af_tab_lo = h.tab_lo; run.af_tab_hi = h.tab_hi;
    if (N <= 1) {                                                           // no pair: every entry empty, no other group
        if (N == 1) {
            h.own_sum[0] = h.near_sum[0] = 0; h.own_lo[0] = h.near_lo[0] = INT32_MAX; h.own_hi[0] = h.near_hi[0] = -1;
            h.near_group[0] = h.near_group[1] = h.near_group[2] = -1;
            for (int b = 0; want && b < G; ++b) { h.tab_sum[b] = 0; h.tab_lo[b] = INT32_MAX; h.tab_hi[b] = -1; }
        }
        return PC_OK;
    }
    const bool cols_pending = run.timed && run.pending;
    if ((rc = slab_finish(c, run, c->last_af_ms, c->h_af.p, c->b_af_out.p, pc_affinity_out_bytes(N, G, want), [&](hipStream_t st) {
            return pc_launch_affinity_finish(c->b_af_tab.p, c->b_af_group.as<int32_t>(), c->b_af_goff.as<int32_t>(), N, G, run.bt_invert, c->b_af_out.p, want, st);
        }))) return rc;
    if (cols_pending) { float y = 0.f; PC_HIP(hipEventElapsedTime(&y, c->ev_slab[1], c->ev_slab[4])); c->last_af_ms[2] += y; }
    if (*h.bad) {
        pc_set_error("%s: %llu values of the fill are no millionth in [0, 1]: the table is not defined on them", run.who, *h.bad);
        return PC_ERR_DATA;
    }
    return PC_OK;
}
// Several devices: a device ships its raw table, 16 N G + 8 bytes, and the root combines the staged ones into its own in one launch
// (k_aff_merge) before it finishes: a pair lies in exactly one stretch, so nothing is counted twice.
size_t PcAffinityFill::ship_bytes(const pc_ctx* root, const PcSlabRun& run) { return pc_affinity_table_bytes(root->dev.N, run.n_groups); }
int PcAffinityFill::ship(pc_ctx* c, pc_ctx* root, PcSlabRun& run, void* stage, int slot, int) {
    int rc = PC_OK;
    const size_t bytes = pc_affinity_table_bytes(c->dev.N, run.n_groups);
    PC_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = pc_ship(c, root, (char*)stage + (size_t)slot * bytes, c->b_af_tab.p, bytes))) return rc;
    PC_HIP(hipEventRecord(c->ev[1], c->stream));
    return PC_OK;
}
int PcAffinityFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float*) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    PC_HIP(hipEventRecord(root->ev[0], root->stream));
    if ((rc = pc_launch_affinity_merge(root->b_af_tab.p, stage, n_foreign, root->dev.N, runs[0].n_groups, root->stream))) return rc;
    PC_HIP(hipEventRecord(root->ev[1], root->stream));
    return PC_OK;
}

extern "C" int pc_fill_affinity(pc_ctx* c, int metric, int as_distance, const int32_t* group, int n_groups, int want_table, int64_t slab_bytes,
                                const int64_t** own_sum, const int32_t** own_lo, const int32_t** own_hi, const int32_t** near_group,
                                const int64_t** near_sum, const int32_t** near_lo, const int32_t** near_hi,
                                const int64_t** tab_sum, const int32_t** tab_lo, const int32_t** tab_hi, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_affinity"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.want_table = want_table != 0; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcAffinityFill>(run, {own_sum, own_lo, own_hi, near_group, near_sum, near_lo, near_hi, tab_sum, tab_lo, tab_hi, n_slabs}, stats,
                                        [&] { return pc_slab_fill<PcAffinityFill>(c, run); });
}

extern "C" int pc_last_affinity_times(const pc_ctx* c, float* ms_rows, float* ms_cols, float* ms_finish) {
    if (!c) { pc_set_error("pc_last_affinity_times: NULL context"); return PC_ERR_ARG; }
    if (ms_rows) *ms_rows = c->last_af_ms[0];
    if (ms_cols) *ms_cols = c->last_af_ms[2];
    if (ms_finish) *ms_finish = c->last_af_ms[1];
    return PC_OK;
}

// ---- distribution fill: the exact histogram of every pair value -- a delivered value is one of the 10^6 + 1 millionths in [0, 1], so
// the whole distribution is pc_hist_bins() integer bins, whatever N is: the count of pairs within ANY threshold (pc_fill_edges' n_edges at
// every threshold at once), every quantile, and the mean, deviation and skewness SymMatrix.statistics takes from the dense matrix
// (matrix.py:132-153).  With a partition two such arrays: class 0 the pairs inside a group, class 1 those between two.  Each filled slab
// goes through ONE pass, k_hist_pass (pc_hist.hip), over a state that stays on the device from the first slab to the last; nothing is
// read back per slab.  After the last slab: k_hist_finish, then one D2H of the bins and the 8-byte violation count behind them.  The walk
// always fills distances, as the between-groups fill's: a similarity histogram is the distance histogram reversed by the finish.  The
// rows form, pc_fill_rows_hist, seeds the state with a stored histogram (PcHistSeed, with the seeds below) and passes the new genomes'
// rows through the rows form of the same pass body: begin and end are these.
int PcHistFill::begin(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int N = c->dev.N, classes = run.group ? 2 : 1;
    const size_t bytes = pc_hist_bytes(classes);
    run.hist_classes = classes; run.hist_pairs = 0;
    if ((rc = slab_begin(c, run, c->last_hist_ms)) || (rc = c->h_hist.ensure(bytes))) return rc;
    if (N <= 1) return PC_OK;
    if ((rc = slab_size(c, run))) return rc;
    if ((rc = c->b_hist_state.ensure(bytes)) || (rc = c->b_hist_out.ensure(bytes))) return abi_rc(rc);
    if (run.group && (rc = upload_raw(c->b_hist_group, run.group, (size_t)N * 4))) return rc;
    PC_HIP(hipMemsetAsync(c->b_hist_state.p, 0, bytes, c->stream));
    return PC_OK;
}
int PcHistFill::slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const PcSlabDomain& dom) {
    if (dom.is_rows != run.rows_form) { pc_set_error("%s: a slab of the other pair domain", run.who); return PC_ERR_ARG; }
    return slab_pass(c, run, c->last_hist_ms, [&](hipStream_t st) {
        return pc_launch_hist_pass(slab, Lp, dom, run.group ? c->b_hist_group.as<int32_t>() : nullptr, run.hist_classes, c->b_hist_state.p, st);
    });
}
int PcHistFill::end(pc_ctx* c, PcSlabRun& run) {
    int rc = PC_OK;
    const int classes = run.hist_classes;
    const size_t words = pc_hist_bytes(classes) / 8;
    int64_t* const h = c->h_hist.as<int64_t>();
    run.hist = h; run.hist_pairs = 0;
    if (c->dev.N <= 1) { memset(h, 0, words * 8); return PC_OK; }            // no pair: every bin zero
    if ((rc = slab_finish(c, run, c->last_hist_ms, h, c->b_hist_out.p, words * 8, [&](hipStream_t st) {
            return pc_launch_hist_finish(c->b_hist_state.p, c->b_hist_out.p, classes, run.bt_invert, st);
        }))) return rc;
    if (h[words - 1]) {
        pc_set_error("%s: %llu values of the fill are no millionth in [0, 1]: the histogram is not defined on them", run.who, (unsigned long long)h[words - 1]);
        return PC_ERR_DATA;
    }
    int64_t total = 0;
    for (size_t i = 0; i + 1 < words; ++i) total += h[i];
    run.hist_pairs = total;
    return PC_OK;
}
// Several devices: a device ships its raw state, pc_hist_bytes(classes), and the root adds the staged ones into its own in one launch
// (k_hist_merge) before it finishes: a pair lies in exactly one stretch, so nothing is counted twice.
size_t PcHistFill::ship_bytes(const pc_ctx*, const PcSlabRun& run) { return pc_hist_bytes(run.group ? 2 : 1); }
int PcHistFill::ship(pc_ctx* c, pc_ctx* root, PcSlabRun& run, void* stage, int slot, int) {
    int rc = PC_OK;
    const size_t bytes = pc_hist_bytes(run.hist_classes);
    PC_HIP(hipEventRecord(c->ev[0], c->stream));
    if ((rc = pc_ship(c, root, (char*)stage + (size_t)slot * bytes, c->b_hist_state.p, bytes))) return rc;
    PC_HIP(hipEventRecord(c->ev[1], c->stream));
    return PC_OK;
}
int PcHistFill::merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float*) {
    int rc = PC_OK;
    pc_ctx* root = ctx[0];
    PC_HIP(hipEventRecord(root->ev[0], root->stream));
    if ((rc = pc_launch_hist_merge(root->b_hist_state.p, stage, n_foreign, runs[0].hist_classes, root->stream))) return rc;
    PC_HIP(hipEventRecord(root->ev[1], root->stream));
    return PC_OK;
}

extern "C" int pc_fill_hist(pc_ctx* c, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                            const int64_t** hist, int32_t* n_classes, int64_t* n_pairs, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_hist"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcHistFill>(run, {hist, n_classes, n_pairs, n_slabs}, stats, [&] { return pc_slab_fill<PcHistFill>(c, run); });
}

extern "C" int pc_last_hist_times(const pc_ctx* c, float* ms_pass, float* ms_finish) {
    return last_times(c, "pc_last_hist_times", c ? c->last_hist_ms : nullptr, ms_pass, ms_finish);
}
extern "C" int pc_hist_bins(void) { return PC_HIST_BINS; }
extern "C" int pc_hist_table_slots(void) { return pc_hist_table_slot_count(); }
extern "C" int pc_hist_probes(void) { return pc_hist_probe_bound(); }

// ---- the rows forms: pc_fill_rows_edges / pc_fill_rows_components / pc_fill_rows_tree / pc_fill_rows_nearest grow a STORED result.  The pairs of the call are
// those that touch a query genome (the new genomes of a grown collection): k query rows cost k N pairs, not N^2 / 2.  What is stored
// stands for the pairs among the other genomes: the components fill takes their labelling as the initial parent[], the tree fill
// their tree's keys as the resident forest (MST(A + B) = MST(MST(A) + B), the invariant the slabs already keep), the nearest fill their
// lists as the resident key[N][K] / nbr[N][K] (the best K of a list and new candidates is the best K of all); a stored edge list
// needs nothing on the device -- the caller merges the two lists.  The same descriptions run: check -> begin -> seed -> the rows walk
// -> end.  The walk cuts the query rows into consecutive ranges of at most max(1, slab_bytes / 8 / N) rows (0: by slab_max_pairs'
// rule), fills each with the rows fill itself (pc_fill_rows_dev) into the context's slab buffer as f64[m][N], and hands it to the
// description's slab() with the PcRowsSlab that says which of its values are pairs of the call.  One slab is resident at a time; the
// rows fill touches no shard state, so the caller's is in force throughout.
static int rows_arg_check(const pc_ctx* c, const char* who, const int32_t* rows, int n_rows) {
    const int N = c->dev.N;
    if (n_rows < 0) { pc_set_error("%s: n_rows %d", who, n_rows); return PC_ERR_ARG; }
    if (n_rows > 0 && !rows) { pc_set_error("%s: rows is NULL", who); return PC_ERR_ARG; }
    for (int k = 0; k < n_rows; ++k)
        if (rows[k] < 0 || rows[k] >= N || (k > 0 && rows[k] <= rows[k - 1])) {
            pc_set_error("%s: rows must be strictly ascending genome indices below %d (rows[%d] = %d)", who, N, k, rows[k]); return PC_ERR_ARG;
        }
    return PC_OK;
}

template <class Fill> static int rows_walk(pc_ctx* c, PcSlabRun& run, const int32_t* rows, int n_rows) {
    int rc = PC_OK;
    const int N = c->dev.N;
    hipStream_t st = c->stream;
    const int per = (int)std::min<int64_t>(std::max<int64_t>(run.max_pairs / N, 1), n_rows);
    if ((rc = c->b_edge_slab.ensure((size_t)per * N * 8))) return abi_rc(rc);
    double* const slab = c->b_edge_slab.as<double>();
    std::vector<int32_t> h_rows(rows, rows + n_rows);
    std::vector<uint8_t> h_query((size_t)N, 0);
    for (int k = 0; k < n_rows; ++k) h_query[rows[k]] = 1;
    if ((rc = wait_last_work(c, st, false)) || (rc = upload_vec(c->b_rq_rows, h_rows)) || (rc = upload_vec(c->b_rq_query, h_query))) return rc;
    for (int r0 = 0; r0 < n_rows; r0 += per) {
        const int m = std::min(per, n_rows - r0);
        pc_stats one; memset(&one, 0, sizeof(one));
        // (the rows fill waits for the pass the slab before it left running before it rewrites the slab and its own tables)
        if ((rc = pc_fill_rows_dev(c, run.metric, run.as_distance, rows + r0, m, slab, st, run.timed ? &one : nullptr))) return rc;
        if (run.timed) pc_stats_add(run.sum, one);
        // test-hooks build only (the release getter answers NULL): the injected rows stand for the slab as filled, every element of it
        int32_t hooked_rows = 0, hooked_n = 0;
        if (const double* const hooked = pc_hooked_rows_values(&hooked_rows, &hooked_n)) {
            if (hooked_rows != n_rows || hooked_n != N) {
                pc_set_error("rows walk: pc_hook_rows_values holds %d rows of %d values, the call has %d query rows of %d genomes", (int)hooked_rows,
                             (int)hooked_n, n_rows, N);
                return PC_ERR_ARG;
            }
            PC_HIP(hipMemcpyAsync(slab, hooked + (size_t)r0 * N, (size_t)m * N * 8, hipMemcpyHostToDevice, st));
        }
        const PcRowsSlab dom{m, N, c->b_rq_rows.as<int32_t>() + r0, c->b_rq_query.as<uint8_t>(), 0, 0};
        if ((rc = Fill::slab(c, run, slab, (int64_t)m * N, dom))) return rc;
        ++run.n_slabs;
    }
    return PC_OK;
}

// A rows form on one context: the refusals in the order of the public calls (pc_slab_check's, the rows argument, the seed), then begin,
// the packed seed onto the device once begin has sized and initialised the state (N > 1 only), the rows walk, end.
template <class Fill> static int pc_rows_slab_fill(pc_ctx* c, PcSlabRun& run, const int32_t* rows, int n_rows, typename Fill::Seed seed) {
    int rc = PC_OK;
    if ((rc = pc_slab_check(c, run, Fill::what)) || (rc = rows_arg_check(c, run.who, rows, n_rows)) || (rc = seed.pack(c, run, rows, n_rows))) return rc;
    PC_ON_DEVICE(c);
    PcRange range(Fill::range);
    run.rows_form = true; run.n_query = n_rows;
    if ((rc = Fill::begin(c, run))) return rc;
    if (c->dev.N > 1) {
        if ((rc = seed.install(c, run))) return rc;
        if (n_rows > 0 && (rc = rows_walk<Fill>(c, run, rows, n_rows))) return rc;
    }
    return Fill::end(c, run);
}

// ---- the seeds (PcNoSeed: pc_host.h) ----
int PcLabelSeed::pack(const pc_ctx* c, const PcSlabRun& run, const int32_t*, int) {
    if (!labels) return PC_OK;
    const int N = c->dev.N;
    packed.resize((size_t)N);
    std::copy(labels, labels + N, packed.begin());
    for (int g = 0; g < N; ++g)
        if (packed[g] < 0 || packed[g] > g || packed[packed[g]] != packed[g]) {
            pc_set_error("%s: seed_labels[%d] = %d is not the smallest member of a component (0 <= label <= genome, a label labels itself)", run.who, g, packed[g]);
            return PC_ERR_ARG;
        }
    return PC_OK;
}
// parent[g] = the stored label, through the pinned labels image (end() rewrites it only after the stream has drained)
int PcLabelSeed::install(pc_ctx* c, PcSlabRun&) const {
    if (packed.empty()) return PC_OK;
    memcpy(c->h_cc_labels.p, packed.data(), packed.size() * 4);
    PC_HIP(hipMemcpyAsync(c->b_cc_parent.p, c->h_cc_labels.p, packed.size() * 4, hipMemcpyHostToDevice, c->stream));
    return PC_OK;
}

int PcTreeSeed::pack(const pc_ctx* c, const PcSlabRun& run, const int32_t*, int) {
    const int N = c->dev.N;
    if (n < 0 || n > std::max(N - 1, 0)) { pc_set_error("%s: %d seed edges for %d genomes (a forest holds at most N - 1)", run.who, n, N); return PC_ERR_ARG; }
    if (n > 0 && !(src && tgt && val)) { pc_set_error("%s: a seed array is NULL", run.who); return PC_ERR_ARG; }
    keys.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double v = val[i], k = __builtin_rint(v * 1.0e6);
        const bool millionth = k >= 0.0 && k <= 1.0e6 && k / 1000000.0 == v;
        const int micro = millionth ? (run.as_distance ? (int)k : PC_TREE_MICRO_MAX - (int)k) : -1;
        keys[i] = tgt[i] < N ? pc_tree_key(micro, src[i], tgt[i]) : PC_TREE_NONE;
        if (keys[i] == PC_TREE_NONE) {
            pc_set_error("%s: seed edge %d (%d, %d, %.17g) is no key: source < target < %d and a value that is a millionth in [0, 1]", run.who, i,
                         src[i], tgt[i], v, N);
            return PC_ERR_ARG;
        }
    }
    return PC_OK;
}
// the stored tree as the resident forest in place of the empty one, through the pinned key image (end() rewrites it after the stream has drained)
int PcTreeSeed::install(pc_ctx* c, PcSlabRun& run) const {
    if (keys.empty()) return PC_OK;
    const int N = c->dev.N;
    unsigned long long* const h = c->h_tree_keys.as<unsigned long long>();
    memcpy(h, keys.data(), keys.size() * 8);
    h[N - 1] = (unsigned long long)keys.size(); h[N] = 0ull; h[N + 1] = 0ull;
    PC_HIP(hipMemcpyAsync(tree_list(c, 0), h, tree_list_words(c) * 8, hipMemcpyHostToDevice, c->stream));
    if (run.n_query > 0) return PC_OK;
    // no query row: one pass over the list alone leaves the tree of the seed edges (a seed that is no forest comes out short, and end() says so)
    return slab_pass(c, run, c->last_tree_ms, [&](hipStream_t st) { return tree_pass(c, run, nullptr, 0, nullptr, nullptr, 0, st); });
}

// The stored lists are seed_nbr / seed_val [N][k_seed] in the uploaded collection's numbering, rows of query genomes ignored: the best
// min(K, N_old - 1) old neighbours of every old genome, N_old = N - n_rows.  They replace the sentinel in the resident lists; the query
// rows' pairs are merged into them by the one total order, so an old genome's list is the best kk of all its N - 1 candidates (every old
// candidate outside the stored list is worse than every entry in it), and a query genome's list is built from its row alone.
int PcNearestSeed::pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows) {
    const int N = c->dev.N, kk = run.kk, n_old = N - n_rows;
    const int need = std::max(std::min(kk, n_old - 1), 0);                  // entries a stored list must hold; more (up to kk) are taken, the rest cut
    if (k_seed < need) {
        pc_set_error("%s: k_seed %d is below min(k, N_old - 1) = %d (%d old genomes): the stored lists cannot decide %d neighbours", run.who, (int)k_seed, need, n_old, kk);
        return PC_ERR_ARG;
    }
    if (n_old > 1 && !(nbr && val)) { pc_set_error("%s: a seed array is NULL with %d old genomes", run.who, n_old); return PC_ERR_ARG; }
    ks = std::min<int>(std::min<int>(k_seed, kk), std::max(n_old - 1, 0));
    if (ks == 0) return PC_OK;
    std::vector<uint8_t> is_query((size_t)N, 0);
    for (int i = 0; i < n_rows; ++i) is_query[rows[i]] = 1;
    keys.resize((size_t)N * kk); idx.resize((size_t)N * kk);
    int bad_g = -1, bad_j = -1;
    const int why = pc_nn_seed_pack(nbr, val, k_seed, ks, N, kk, is_query.data(), run.as_distance, keys.data(), idx.data(), &bad_g, &bad_j);
    if (why) {
        pc_set_error("%s: seed entry [%d][%d] = (%d, %.17g) %s", run.who, bad_g, bad_j, nbr[(size_t)bad_g * k_seed + bad_j], val[(size_t)bad_g * k_seed + bad_j],
                     why == 1 ? "is no other old genome (out of range, a query genome, or the genome itself)"
                              : "does not come after the entry before it: a stored list ascends in (value, better first; then index)");
        return PC_ERR_ARG;
    }
    return PC_OK;
}
// the stored lists in place of the sentinel, through the pinned result image (end() rewrites it only after the stream has drained)
int PcNearestSeed::install(pc_ctx* c, PcSlabRun& run) const {
    if (ks == 0) return PC_OK;
    const size_t n_ent = nn_entries(c, run);
    memcpy(c->h_nn.p, keys.data(), n_ent * 8);
    memcpy((char*)c->h_nn.p + n_ent * 8, idx.data(), n_ent * 4);
    PC_HIP(hipMemcpyAsync(c->b_nn_key.p, c->h_nn.p, n_ent * 8, hipMemcpyHostToDevice, c->stream));
    PC_HIP(hipMemcpyAsync(nn_nbr(c, run), (const char*)c->h_nn.p + n_ent * 8, n_ent * 4, hipMemcpyHostToDevice, c->stream));
    return PC_OK;
}

// The stored table is the caller's four [G][G] arrays in the result layout and the call's direction.  pack holds every entry to what a
// fill of `group` over the genomes that are no query rows delivers -- symmetric, empty or full consistently, 0 <= lo <= hi <= 10^6,
// count lo <= sum <= count hi, and the count the partition's own: old[a] old[b] pairs between two groups, old[a] (old[a] - 1) / 2
// within one, old[] counting the labelled genomes that are no query -- and packs it as the raw accumulator's image: distances (a
// similarity seed is complemented: the walk fills distances and the fold inverts back), entries a <= b, the rest empty, so that the
// fold returns the seed when no row follows.
int PcBetweenSeed::pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows) {
    const int given = (sum != nullptr) + (count != nullptr) + (lo != nullptr) + (hi != nullptr);
    if (given == 0) return PC_OK;
    if (given != 4) { pc_set_error("%s: %d of the four seed arrays are given (all of seed_sum, seed_count, seed_lo, seed_hi, or none)", run.who, given); return PC_ERR_ARG; }
    const int N = c->dev.N, G = run.n_groups;
    const size_t gg = (size_t)G * (size_t)G;
    std::vector<uint8_t> is_query((size_t)std::max(N, 1), 0);
    for (int k = 0; k < n_rows; ++k) is_query[rows[k]] = 1;
    std::vector<int64_t> old((size_t)G, 0);
    for (int g = 0; g < N; ++g) if (run.group[g] >= 0 && !is_query[g]) ++old[run.group[g]];
    image.assign(pc_between_bytes(G) / 8, 0ull);
    const PcBetweenAcc img = pc_between_view(image.data(), G);
    for (size_t i = 0; i < gg; ++i) img.lo[i] = ~0u;
    for (int a = 0; a < G; ++a)
        for (int b = a; b < G; ++b) {
            const size_t at = (size_t)a * G + b, mirror = (size_t)b * G + a;
            const int64_t s = sum[at], n = count[at];
            const int32_t l = lo[at], h = hi[at];
            const char* why = nullptr;
            if (sum[mirror] != s || count[mirror] != n || lo[mirror] != l || hi[mirror] != h) why = "is not symmetric";
            else if (n < 0 || (n == 0) != (s == 0 && l == INT32_MAX && h == -1) || (n != 0 && (l == INT32_MAX || h == -1)))
                why = "is neither empty (count 0, sum 0, lo INT32_MAX, hi -1) nor full";
            else if (n && (l < 0 || h > 1000000 || l > h)) why = "does not hold 0 <= lo <= hi <= 10^6";
            if (why) {
                pc_set_error("%s: seed entry [%d][%d] (count %lld, sum %lld, lo %d, hi %d) %s", run.who, a, b, (long long)n, (long long)s, (int)l, (int)h, why);
                return PC_ERR_ARG;
            }
            const int64_t want = a == b ? old[a] * (old[a] - 1) / 2 : old[a] * old[b];
            if (n != want) {
                pc_set_error("%s: seed entry [%d][%d] counts %lld pairs, the partition has %lld there (%lld and %lld genomes that are no query rows): "
                             "the stored table is of another partition or another genome set", run.who, a, b, (long long)n, (long long)want,
                             (long long)old[a], (long long)old[b]);
                return PC_ERR_ARG;
            }
            if (!n) continue;
            if ((__int128)s < (__int128)n * l || (__int128)s > (__int128)n * h) {
                pc_set_error("%s: seed entry [%d][%d] (count %lld, sum %lld, lo %d, hi %d) holds a sum outside [count lo, count hi]", run.who, a, b, (long long)n,
                             (long long)s, (int)l, (int)h);
                return PC_ERR_ARG;
            }
            img.cnt[at] = (unsigned long long)n;
            if (run.bt_invert) { img.sum[at] = (unsigned long long)(n * 1000000 - s); img.lo[at] = (uint32_t)(1000000 - h); img.hi[at] = (uint32_t)(1000000 - l); }
            else { img.sum[at] = (unsigned long long)s; img.lo[at] = (uint32_t)l; img.hi[at] = (uint32_t)h; }
        }
    return PC_OK;
}
// the stored table in place of the empty accumulator, through the pinned result image (end() rewrites it only after the stream has drained)
int PcBetweenSeed::install(pc_ctx* c, PcSlabRun& run) const {
    if (image.empty()) return PC_OK;
    const size_t bytes = pc_between_bytes(run.n_groups);
    memcpy(c->h_bt.p, image.data(), bytes);
    PC_HIP(hipMemcpyAsync(c->b_bt_acc.p, c->h_bt.p, bytes, hipMemcpyHostToDevice, c->stream));
    return PC_OK;
}

// A stored histogram as the state's bins: i64[classes][PC_HIST_BINS] in the call's direction (a similarity seed is reversed: the walk
// fills distances and the finish reverses back).  It must be the histogram of the pairs among the genomes that are no query rows: no
// bin negative, the total their N_old (N_old - 1) / 2 pairs, and with a partition class 0 the pairs inside their groups.  (Necessary,
// not sufficient: a histogram cannot name its pairs.)
int PcHistSeed::pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows) {
    if (!hist) return PC_OK;
    const int N = c->dev.N, classes = run.group ? 2 : 1;
    const size_t words = pc_hist_bytes(classes) / 8;
    int64_t total[2] = {0, 0};
    for (int cl = 0; cl < classes; ++cl)
        for (size_t k = 0; k < PC_HIST_BINS; ++k) {
            const int64_t x = hist[(size_t)cl * PC_HIST_BINS + k];
            if (x < 0) { pc_set_error("%s: seed bin [%d][%zu] is negative (%lld)", run.who, cl, k, (long long)x); return PC_ERR_ARG; }
            total[cl] += x;
        }
    std::vector<uint8_t> is_query((size_t)std::max(N, 1), 0);
    for (int k = 0; k < n_rows; ++k) is_query[rows[k]] = 1;
    const int64_t n_old = (int64_t)N - n_rows, want = n_old * (n_old - 1) / 2;
    if (total[0] + total[1] != want) {
        pc_set_error("%s: the seed counts %lld pairs, the %lld genomes that are no query rows have %lld: the stored histogram is of another genome set",
                     run.who, (long long)(total[0] + total[1]), (long long)n_old, (long long)want);
        return PC_ERR_ARG;
    }
    if (run.group) {
        std::vector<int64_t> old((size_t)run.n_groups, 0);
        for (int g = 0; g < N; ++g) if (!is_query[g]) ++old[run.group[g]];
        int64_t within = 0;
        for (int64_t n : old) within += n * (n - 1) / 2;
        if (total[0] != within) {
            pc_set_error("%s: class 0 of the seed counts %lld pairs, the partition has %lld inside its groups over the genomes that are no query rows: "
                         "the stored histogram is of another partition or another genome set", run.who, (long long)total[0], (long long)within);
            return PC_ERR_ARG;
        }
    }
    image.assign(words, 0ull);
    for (int cl = 0; cl < classes; ++cl)
        for (size_t k = 0; k < PC_HIST_BINS; ++k)
            image[(size_t)cl * PC_HIST_BINS + (run.bt_invert ? PC_HIST_BINS - 1 - k : k)] = (unsigned long long)hist[(size_t)cl * PC_HIST_BINS + k];
    return PC_OK;
}
// the stored histogram in place of the empty state, through the pinned result image (end() rewrites it only after the stream has drained)
int PcHistSeed::install(pc_ctx* c, PcSlabRun& run) const {
    if (image.empty()) return PC_OK;
    const size_t bytes = pc_hist_bytes(run.hist_classes);
    memcpy(c->h_hist.p, image.data(), bytes);
    PC_HIP(hipMemcpyAsync(c->b_hist_state.p, c->h_hist.p, bytes, hipMemcpyHostToDevice, c->stream));
    return PC_OK;
}

extern "C" int pc_fill_rows_edges(pc_ctx* c, int metric, int as_distance, double threshold, const int32_t* rows, int n_rows, int64_t slab_bytes,
                                  const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_edges"; run.metric = metric; run.as_distance = as_distance; run.threshold = threshold; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcEdgesFill>(run, {src, tgt, val, n_edges, n_slabs}, stats, [&] { return pc_rows_slab_fill<PcEdgesFill>(c, run, rows, n_rows, {}); });
}

extern "C" int pc_fill_rows_components(pc_ctx* c, int metric, int as_distance, double threshold, int strict, const int32_t* rows, int n_rows,
                                       const int32_t* seed_labels, int64_t slab_bytes, const int32_t** labels, int32_t* n_components, int64_t* n_edges,
                                       int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_components"; run.metric = metric; run.as_distance = as_distance; run.strict = strict; run.threshold = threshold;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcComponentsFill>(run, {labels, n_components, n_edges, n_slabs}, stats,
                                          [&] { return pc_rows_slab_fill<PcComponentsFill>(c, run, rows, n_rows, {seed_labels}); });
}

extern "C" int pc_fill_rows_tree(pc_ctx* c, int metric, int as_distance, const int32_t* rows, int n_rows, const int32_t* seed_src, const int32_t* seed_tgt,
                                 const double* seed_val, int32_t n_seed, int64_t slab_bytes, const int32_t** src, const int32_t** tgt, const double** val,
                                 int32_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_tree"; run.metric = metric; run.as_distance = as_distance; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcTreeFill>(run, {src, tgt, val, n_edges, n_slabs}, stats,
                                    [&] { return pc_rows_slab_fill<PcTreeFill>(c, run, rows, n_rows, {seed_src, seed_tgt, seed_val, n_seed}); });
}

extern "C" int pc_fill_rows_nearest(pc_ctx* c, int metric, int as_distance, int k, const int32_t* rows, int n_rows, const int32_t* seed_nbr,
                                    const double* seed_val, int32_t k_seed, int64_t slab_bytes, const int32_t** nbr, const double** val, int32_t* k_out,
                                    int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_nearest"; run.metric = metric; run.as_distance = as_distance; run.k = k; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcNearestFill>(run, {nbr, val, k_out, n_slabs}, stats,
                                       [&] { return pc_rows_slab_fill<PcNearestFill>(c, run, rows, n_rows, {seed_nbr, seed_val, k_seed}); });
}

// The rows form of the affinity fill: nothing stored is needed on the device (PcNoSeed) -- the stored partition is `group` itself; what
// the queries add to the stored own entries is delivered (want_gain) and combined by the caller.  The walk fills distances, as the whole form's.
extern "C" int pc_fill_rows_affinity(pc_ctx* c, int metric, int as_distance, const int32_t* group, int n_groups, const int32_t* rows, int n_rows,
                                     int want_table, int want_gain, int64_t slab_bytes,
                                     const int64_t** own_sum, const int32_t** own_lo, const int32_t** own_hi, const int32_t** near_group,
                                     const int64_t** near_sum, const int32_t** near_lo, const int32_t** near_hi,
                                     const int64_t** tab_sum, const int32_t** tab_lo, const int32_t** tab_hi,
                                     const int64_t** gain_sum, const int32_t** gain_lo, const int32_t** gain_hi, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_affinity"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.allow_unlabelled = true; run.query = rows; run.want_table = want_table != 0; run.want_gain = want_gain != 0; run.slab_bytes = slab_bytes;
    const PcPlacementOut out{{own_sum, own_lo, own_hi, near_group, near_sum, near_lo, near_hi, tab_sum, tab_lo, tab_hi, n_slabs}, gain_sum, gain_lo, gain_hi};
    return pc_slab_call<PcAffinityFill, PcPlacementOut>(run, out, stats, [&] { return pc_rows_slab_fill<PcAffinityFill>(c, run, rows, n_rows, {}); });
}

// The rows form of the between-groups fill: the stored table (PcBetweenSeed) and the pairs that have a query genome at one end are the
// table of the grown collection, integer for integer -- counts and sums add, extremes only move outward.  Without a seed: the table over
// those pairs alone.  A label may be -1 (a member of no group: in no pair).  The walk fills distances, as the whole form's.
extern "C" int pc_fill_rows_between(pc_ctx* c, int metric, int as_distance, const int32_t* group, int n_groups, const int32_t* rows, int n_rows,
                                    const int64_t* seed_sum, const int64_t* seed_count, const int32_t* seed_lo, const int32_t* seed_hi, int64_t slab_bytes,
                                    const int64_t** sum, const int64_t** count, const int32_t** lo, const int32_t** hi, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_between"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.allow_unlabelled = true; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcBetweenFill>(run, {sum, count, lo, hi, n_slabs}, stats,
                                       [&] { return pc_rows_slab_fill<PcBetweenFill>(c, run, rows, n_rows, {seed_sum, seed_count, seed_lo, seed_hi}); });
}

// The rows form of the distribution fill: the stored histogram (PcHistSeed) and the pairs that have a query genome at one end, each once,
// are the histogram of the grown collection, bin for bin -- counts add.  Without a seed: the histogram over those pairs alone.  Every
// genome is labelled (this form keeps to full partitions: a label of -1 is refused).  The walk fills distances, as the whole form's.
extern "C" int pc_fill_rows_hist(pc_ctx* c, int metric, int as_distance, const int32_t* group, int n_groups, const int32_t* rows, int n_rows,
                                 const int64_t* seed_hist, int64_t slab_bytes, const int64_t** hist, int32_t* n_classes, int64_t* n_pairs, int32_t* n_slabs,
                                 pc_stats* stats) {
    PcSlabRun run; run.who = "pc_fill_rows_hist"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcHistFill>(run, {hist, n_classes, n_pairs, n_slabs}, stats, [&] { return pc_rows_slab_fill<PcHistFill>(c, run, rows, n_rows, {seed_hist}); });
}

// elements one workgroup of a slab pass covers (0: edge count / emit, 1: union, 2: tree scan): what a test of the passes' seams sizes its slabs by
extern "C" int pc_rows_pass_span(int pass_kind) { return pc_rows_slab_span(pass_kind); }
// the tile edge of the nearest-neighbours rows form's column pass (rows and columns): what a test of its seams sizes its inputs by
extern "C" int pc_nearest_rows_tile(void) { return pc_nn_rows_tile(); }
