// pc_fill_slabs.hip -- the fills of libphamclust_hip.so that walk the matrix slab by slab and deliver what a threshold leaves of it:
// pc_fill_edges (the passing pairs as an edge list) and pc_fill_components (their connected components), with pc_last_edge_times and
// pc_last_component_times -- and, on the same walk without a threshold, pc_fill_nearest (every genome's k best neighbours) with
// pc_last_nearest_times.  Host only.
//
// The walk they share goes over successive contiguous ranges of target genomes ("slabs": pc_chunk_plan over count[t] = t under
// slab_bytes / 8 pairs, at most 2^31-1 so that u32 counts and offsets do); each range is installed as a PcShard (owned = t0 .. t1-1,
// shard-local layout), filled by fill_impl into the context's slab buffer and handed to the caller's hook.  Slabs come in ascending target
// order; one slab is resident at a time.
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

// The checks the calls make, after fill_check's (pc_fill_nearest has no threshold and passes 0); outputs: every output pointer is there
static int slab_check(const pc_ctx* c, const char* who, bool outputs, int metric, double threshold, int64_t slab_bytes) {
    if (!outputs) { pc_set_error("%s: an output pointer is NULL", who); return PC_ERR_ARG; }
    if (threshold != threshold) { pc_set_error("%s: the threshold is NaN", who); return PC_ERR_ARG; }
    if (slab_bytes < 0) { pc_set_error("%s: slab_bytes %lld", who, (long long)slab_bytes); return PC_ERR_ARG; }
    return fill_check_residues(c, who, metric);
}

// The cut (N > 1): ranges of targets whose pairs fit the slab, range starts followed by N, and the slab buffer sized for the largest.
// slab_bytes == 0: the dense triangle, or a quarter of what is free now (an aai / peq slab's plan takes its own half) -- so this runs
// before the call allocates anything of its own.
static int slab_cut(pc_ctx* c, int64_t slab_bytes, std::vector<int32_t>& cut) {
    const int N = c->dev.N;
    int64_t max_pairs;
    if (slab_bytes > 0) max_pairs = std::max<int64_t>(slab_bytes / 8, 1);
    else {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
        max_pairs = std::min<int64_t>(pairs_below(N), std::max<int64_t>((int64_t)((free_b + c->b_edge_slab.cap) / 4 / 8), 1));
    }
    max_pairs = std::min<int64_t>(max_pairs, PC_EDGE_MAX_PAIRS);
    std::vector<uint64_t> per_target((size_t)N);
    for (int t = 0; t < N; ++t) per_target[t] = (uint64_t)t;
    const int nsl = pc_chunk_plan(per_target.data(), N, (uint64_t)max_pairs, nullptr, 0);
    if (nsl < 0) return nsl;
    cut.resize((size_t)nsl + 1);
    int rc = PC_OK;
    if ((rc = pc_chunk_plan(per_target.data(), N, (uint64_t)max_pairs, cut.data(), nsl + 1)) < 0) return rc;
    int64_t most = 1;
    for (int i = 0; i < nsl; ++i) most = std::max(most, pairs_below(cut[i + 1]) - pairs_below(cut[i]));
    return abi_rc(c->b_edge_slab.ensure((size_t)most * 8));
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
        if ((rc = hook(slab, Lp, c->shard))) return rc;
    }
    return PC_OK;
}

// ---- edge-list fill: the pairs whose value passes a threshold, as (source, target, value) arrays sorted by target, then source --
// what matrix_to_adjacency(skip_zero) writes and SymMatrix.nearest_neighbors answers from the dense matrix (matrix.py:536-551,
// 265-296), without the dense matrix ever crossing PCIe.  Each filled slab is compacted (count -> scan -> one 4-byte read-back -> emit,
// pc_edges.hip) and its edges appended to the pinned host result; slabs in ascending target order make the concatenation globally ordered.
extern "C" int pc_fill_edges(pc_ctx* c, int metric, int as_distance, double threshold, int64_t slab_bytes,
                             const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    if (src) *src = nullptr;
    if (tgt) *tgt = nullptr;
    if (val) *val = nullptr;
    if (n_edges) *n_edges = 0;
    if (n_slabs) *n_slabs = 0;
    int rc = PC_OK;
    if ((rc = fill_check(c, "pc_fill_edges", "an edge-list fill", &metric, nullptr)) ||
        (rc = slab_check(c, "pc_fill_edges", src && tgt && val && n_edges && n_slabs, metric, threshold, slab_bytes))) return rc;
    PC_ON_DEVICE(c);
    PcRange range("pc:fill_edges");
    hipStream_t st = c->stream;
    pc_stats sum; memset(&sum, 0, sizeof(sum));
    c->last_edge_ms[0] = c->last_edge_ms[1] = 0.f;
    as_distance = as_distance ? 1 : 0;
    if ((rc = wait_last_work(c, st, false))) return rc;                     // (the loan of an earlier call ends here: its buffers are rewritten)
    if ((rc = c->h_edge_src.ensure(16)) || (rc = c->h_edge_tgt.ensure(16)) || (rc = c->h_edge_val.ensure(16))) return rc;
    if (c->dev.N <= 1) {
        *src = c->h_edge_src.as<int32_t>(); *tgt = c->h_edge_tgt.as<int32_t>(); *val = c->h_edge_val.as<double>();
        if (stats) *stats = sum;
        return PC_OK;
    }
    std::vector<int32_t> cut;
    if ((rc = slab_cut(c, slab_bytes, cut))) return rc;
    if (stats) for (hipEvent_t& e : c->ev_edge) if (!e) PC_HIP(hipEventCreate(&e));
    uint32_t* const h_total = c->h_plan.as<uint32_t>();
    int64_t E = 0;
    // ---- a slab's hook, compact: count -> scan (n + 1 elements: the total falls out) -> read the total back -> emit
    rc = slab_walk(c, cut, metric, as_distance, stats ? &sum : nullptr, [&](const double* slab, int64_t Lp, const PcShard& shard) -> int {
        int rc = PC_OK;
        const int64_t nch = pc_edge_chunks(Lp);
        if ((rc = c->b_edge_cnt.ensure((size_t)(nch + 1) * 4)) || (rc = c->b_edge_off.ensure((size_t)(nch + 1) * 4)) ||
            (rc = c->b_scan_tmp.ensure((size_t)pc_scan_tmp_elems(nch + 1) * 4))) return abi_rc(rc);
        uint32_t* const cnt = c->b_edge_cnt.as<uint32_t>(); uint32_t* const off = c->b_edge_off.as<uint32_t>();
        if (stats) PC_HIP(hipEventRecord(c->ev_edge[0], st));
        PC_HIP(hipMemsetAsync(cnt + nch, 0, 4, st));
        if ((rc = pc_launch_edge_count(slab, Lp, as_distance, threshold, cnt, st))) return rc;
        if ((rc = pc_scan_exclusive_u32(cnt, off, nch + 1, c->b_scan_tmp.as<uint32_t>(), (int64_t)(c->b_scan_tmp.cap / 4), st))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_edge[1], st));
        PC_HIP(hipMemcpyAsync(h_total, off + nch, 4, hipMemcpyDeviceToHost, st));
        PC_HIP(hipStreamSynchronize(st));
        c->busy = false;
        const int64_t Es = (int64_t)h_total[0];
        if (Es == 0) {
            if (stats) { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, c->ev_edge[0], c->ev_edge[1])); c->last_edge_ms[0] += x; }
            return PC_OK;
        }
        if ((rc = c->b_edge_src.ensure((size_t)Es * 4)) || (rc = c->b_edge_tgt.ensure((size_t)Es * 4)) || (rc = c->b_edge_val.ensure((size_t)Es * 8))) return abi_rc(rc);
        if ((rc = c->h_edge_src.grow_keep((size_t)(E + Es) * 4, (size_t)E * 4)) || (rc = c->h_edge_tgt.grow_keep((size_t)(E + Es) * 4, (size_t)E * 4)) ||
            (rc = c->h_edge_val.grow_keep((size_t)(E + Es) * 8, (size_t)E * 8))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_edge[2], st));
        if ((rc = pc_launch_edge_emit(slab, Lp, as_distance, threshold, shard, off, c->b_edge_src.as<int32_t>(), c->b_edge_tgt.as<int32_t>(),
                                      c->b_edge_val.as<double>(), st))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_edge[3], st));
        PC_HIP(hipMemcpyAsync(c->h_edge_src.as<int32_t>() + E, c->b_edge_src.p, (size_t)Es * 4, hipMemcpyDeviceToHost, st));
        PC_HIP(hipMemcpyAsync(c->h_edge_tgt.as<int32_t>() + E, c->b_edge_tgt.p, (size_t)Es * 4, hipMemcpyDeviceToHost, st));
        PC_HIP(hipMemcpyAsync(c->h_edge_val.as<double>() + E, c->b_edge_val.p, (size_t)Es * 8, hipMemcpyDeviceToHost, st));
        if (stats) PC_HIP(hipEventRecord(c->ev_edge[4], st));
        PC_HIP(hipStreamSynchronize(st));                                   // the slab, its tables and the edge buffers are rewritten by the next range
        if (stats) {
            float x = 0.f, y = 0.f, z = 0.f;
            PC_HIP(hipEventElapsedTime(&x, c->ev_edge[0], c->ev_edge[1]));
            PC_HIP(hipEventElapsedTime(&y, c->ev_edge[2], c->ev_edge[3]));
            PC_HIP(hipEventElapsedTime(&z, c->ev_edge[3], c->ev_edge[4]));
            c->last_edge_ms[0] += x + y; c->last_edge_ms[1] += z;
        }
        E += Es;
        return PC_OK;
    });
    if (rc != PC_OK) return rc;
    *src = c->h_edge_src.as<int32_t>(); *tgt = c->h_edge_tgt.as<int32_t>(); *val = c->h_edge_val.as<double>();
    *n_edges = E; *n_slabs = (int32_t)cut.size() - 1;
    if (stats) *stats = sum;
    return PC_OK;
}

extern "C" int pc_last_edge_times(const pc_ctx* c, float* ms_compact, float* ms_d2h) {
    if (!c) { pc_set_error("pc_last_edge_times: NULL context"); return PC_ERR_ARG; }
    if (ms_compact) *ms_compact = c->last_edge_ms[0];
    if (ms_d2h) *ms_d2h = c->last_edge_ms[1];
    return PC_OK;
}

// ---- components fill: the connected components of the graph {pairs that pass the threshold} -- with a strict distance predicate the
// reference's single-linkage clusters at that eps (clustering.py:4-51) -- as labels[N], the smallest member's index.  Each filled slab
// goes through ONE pass, k_cc_union (pc_components.hip), over a parent[N] array that stays on the device from the first slab to the
// last; nothing is read back per slab.  After the last slab: k_cc_labels, then one D2H of labels[N] and the 8-byte count of passing
// pairs behind them.
extern "C" int pc_fill_components(pc_ctx* c, int metric, int as_distance, double threshold, int strict, int64_t slab_bytes,
                                  const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    if (labels) *labels = nullptr;
    if (n_components) *n_components = 0;
    if (n_edges) *n_edges = 0;
    if (n_slabs) *n_slabs = 0;
    int rc = PC_OK;
    if ((rc = fill_check(c, "pc_fill_components", "a components fill", &metric, nullptr)) ||
        (rc = slab_check(c, "pc_fill_components", labels && n_components && n_edges && n_slabs, metric, threshold, slab_bytes))) return rc;
    PC_ON_DEVICE(c);
    PcRange range("pc:fill_components");
    hipStream_t st = c->stream;
    const int N = c->dev.N;
    pc_stats sum; memset(&sum, 0, sizeof(sum));
    c->last_cc_ms[0] = c->last_cc_ms[1] = 0.f;
    as_distance = as_distance ? 1 : 0; strict = strict ? 1 : 0;
    if ((rc = wait_last_work(c, st, false))) return rc;                     // (the loan of an earlier call ends here: its buffer is rewritten)
    const size_t label_bytes = ((size_t)std::max(N, 1) * 4 + 7) / 8 * 8;    // the 64-bit count sits behind the labels, aligned
    if ((rc = c->h_cc_labels.ensure(label_bytes + 8))) return rc;
    int32_t* const h_labels = c->h_cc_labels.as<int32_t>();
    if (N <= 1) {
        if (N == 1) { h_labels[0] = 0; *n_components = 1; }
        *labels = h_labels;
        if (stats) *stats = sum;
        return PC_OK;
    }
    std::vector<int32_t> cut;
    if ((rc = slab_cut(c, slab_bytes, cut))) return rc;
    if ((rc = c->b_cc_parent.ensure((size_t)N * 4)) || (rc = c->b_cc_labels.ensure(label_bytes + 8))) return abi_rc(rc);
    if (stats) for (hipEvent_t& e : c->ev_cc) if (!e) PC_HIP(hipEventCreate(&e));
    int32_t* const parent = c->b_cc_parent.as<int32_t>();
    unsigned long long* const d_pass = (unsigned long long*)((char*)c->b_cc_labels.p + label_bytes);
    if ((rc = pc_launch_cc_init(parent, N, d_pass, st))) return rc;
    bool pending = false;                                                   // a union pass was launched and, with stats, its time not yet added
    auto add_union_time = [&]() -> int { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, c->ev_cc[0], c->ev_cc[1])); c->last_cc_ms[0] += x; return PC_OK; };
    // ---- a slab's hook: the union pass, left running (the walk has waited for the pass before it: its two events can be read)
    rc = slab_walk(c, cut, metric, as_distance, stats ? &sum : nullptr, [&](const double* slab, int64_t Lp, const PcShard& shard) -> int {
        int rc = PC_OK;
        if (stats && pending && (rc = add_union_time())) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_cc[0], st));
        if ((rc = pc_launch_cc_union(slab, Lp, as_distance, strict, threshold, shard, parent, d_pass, st))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_cc[1], st));
        pending = true;
        return mark_work(c, st);
    });
    if (rc != PC_OK) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_cc[2], st));
    if ((rc = pc_launch_cc_labels(parent, c->b_cc_labels.as<int32_t>(), N, st))) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_cc[3], st));
    PC_HIP(hipMemcpyAsync(h_labels, c->b_cc_labels.p, label_bytes + 8, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    if (stats) {
        if (pending && (rc = add_union_time())) return rc;                  // (the last slab's pass)
        PC_HIP(hipEventElapsedTime(&c->last_cc_ms[1], c->ev_cc[2], c->ev_cc[3]));
    }
    int32_t comps = 0;
    for (int g = 0; g < N; ++g) comps += h_labels[g] == g;
    unsigned long long passed = 0;
    memcpy(&passed, (const char*)h_labels + label_bytes, 8);
    *labels = h_labels; *n_components = comps; *n_edges = (int64_t)passed; *n_slabs = (int32_t)cut.size() - 1;
    if (stats) *stats = sum;
    return PC_OK;
}

extern "C" int pc_last_component_times(const pc_ctx* c, float* ms_union, float* ms_labels) {
    if (!c) { pc_set_error("pc_last_component_times: NULL context"); return PC_ERR_ARG; }
    if (ms_union) *ms_union = c->last_cc_ms[0];
    if (ms_labels) *ms_labels = c->last_cc_ms[1];
    return PC_OK;
}

// ---- nearest-neighbours fill: each genome's k best neighbours in the total order (value, better first; then index) -- what
// SymMatrix.nearest_neighbors answers per node from the dense matrix (matrix.py:265-296), cut after k -- as nbr[N][kk], val[N][kk].
// Each filled slab goes through two passes (pc_nearest.hip: k_nn_rows, k_nn_cols) over key[N][kk] / nbr[N][kk], which stay on the
// device from the first slab to the last; nothing is read back per slab.  After the last slab: k_nn_finish, then one D2H of
// val[N][kk] with nbr[N][kk] behind it.
extern "C" int pc_fill_nearest(pc_ctx* c, int metric, int as_distance, int k, int64_t slab_bytes,
                               const int32_t** nbr, const double** val, int32_t* k_out, int32_t* n_slabs, pc_stats* stats) {
    if (nbr) *nbr = nullptr;
    if (val) *val = nullptr;
    if (k_out) *k_out = 0;
    if (n_slabs) *n_slabs = 0;
    int rc = PC_OK;
    if ((rc = fill_check(c, "pc_fill_nearest", "a nearest-neighbours fill", &metric, nullptr))) return rc;
    if (k < 1) { pc_set_error("pc_fill_nearest: k %d", k); return PC_ERR_ARG; }
    if (k > PC_NEAREST_MAX_K) { pc_set_error("pc_fill_nearest: k %d is above PC_NEAREST_MAX_K = %d", k, PC_NEAREST_MAX_K); return PC_ERR_LIMIT; }
    if ((rc = slab_check(c, "pc_fill_nearest", nbr && val && k_out && n_slabs, metric, 0.0, slab_bytes))) return rc;
    PC_ON_DEVICE(c);
    PcRange range("pc:fill_nearest");
    hipStream_t st = c->stream;
    const int N = c->dev.N;
    const int kk = std::max(std::min(k, N - 1), 0);
    const size_t n_ent = (size_t)std::max(N, 0) * kk, val_bytes = n_ent * 8, out_bytes = val_bytes + n_ent * 4;
    pc_stats sum; memset(&sum, 0, sizeof(sum));
    c->last_nn_ms[0] = c->last_nn_ms[1] = 0.f;
    as_distance = as_distance ? 1 : 0;
    if ((rc = wait_last_work(c, st, false))) return rc;                     // (the loan of an earlier call ends here: its buffer is rewritten)
    if ((rc = c->h_nn.ensure(std::max<size_t>(out_bytes, 16)))) return rc;
    const double* const h_val = c->h_nn.as<double>();
    const int32_t* const h_nbr = (const int32_t*)((const char*)c->h_nn.p + val_bytes);
    if (N <= 1) {
        *nbr = h_nbr; *val = h_val;
        if (stats) *stats = sum;
        return PC_OK;
    }
    std::vector<int32_t> cut;
    if ((rc = slab_cut(c, slab_bytes, cut))) return rc;
    if ((rc = c->b_nn_key.ensure(n_ent * 8)) || (rc = c->b_nn_out.ensure(out_bytes))) return abi_rc(rc);
    if (stats) for (hipEvent_t& e : c->ev_nn) if (!e) PC_HIP(hipEventCreate(&e));
    unsigned long long* const d_key = c->b_nn_key.as<unsigned long long>();
    double* const d_val = c->b_nn_out.as<double>();
    int32_t* const d_nbr = (int32_t*)((char*)c->b_nn_out.p + val_bytes);
    if ((rc = pc_launch_nn_init(d_key, d_nbr, (int64_t)n_ent, st))) return rc;
    bool pending = false;                                                   // a slab's passes were launched and, with stats, their time not yet added
    auto add_select_time = [&]() -> int { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, c->ev_nn[0], c->ev_nn[1])); c->last_nn_ms[0] += x; return PC_OK; };
    // ---- a slab's hook: the row pass, then the column pass, left running (the walk has waited for the passes before them: their two
    // events can be read).  The slab's targets are the consecutive range that starts at its first owned one.
    rc = slab_walk(c, cut, metric, as_distance, stats ? &sum : nullptr, [&](const double* slab, int64_t Lp, const PcShard& shard) -> int {
        int rc = PC_OK;
        const int t0 = c->h_owned[0], t1 = t0 + shard.nown;
        if (stats && pending && (rc = add_select_time())) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_nn[0], st));
        if ((rc = pc_launch_nn_select(slab, Lp, t0, t1, as_distance, kk, d_key, d_nbr, st))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_nn[1], st));
        pending = true;
        return mark_work(c, st);
    });
    if (rc != PC_OK) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_nn[2], st));
    if ((rc = pc_launch_nn_finish(d_key, d_val, (int64_t)n_ent, as_distance, st))) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_nn[3], st));
    PC_HIP(hipMemcpyAsync(c->h_nn.p, c->b_nn_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    if (stats) {
        if (pending && (rc = add_select_time())) return rc;                 // (the last slab's passes)
        PC_HIP(hipEventElapsedTime(&c->last_nn_ms[1], c->ev_nn[2], c->ev_nn[3]));
    }
    *nbr = h_nbr; *val = h_val; *k_out = kk; *n_slabs = (int32_t)cut.size() - 1;
    if (stats) *stats = sum;
    return PC_OK;
}

extern "C" int pc_last_nearest_times(const pc_ctx* c, float* ms_select, float* ms_finish) {
    if (!c) { pc_set_error("pc_last_nearest_times: NULL context"); return PC_ERR_ARG; }
    if (ms_select) *ms_select = c->last_nn_ms[0];
    if (ms_finish) *ms_finish = c->last_nn_ms[1];
    return PC_OK;
}
