// pc_multi.hip -- one process, several GPUs: the pc_multi_* entry points of libphamclust_hip.so.
#include <cstdio>
#include <new>
#include <string>

#include "pc_host.h"

// ---------------------------------------------------------------------------------------------------------------------
// One process, several GPUs ("pc_ctx_create(out, device_ids, n_dev) ... the library owns one host thread per
// GPU ... invisible to Python").  The torch.distributed route (one PROCESS per GPU, pc_set_shard* + the caller's RCCL gather) costs
// ~2.5 s before the first pair -- a launcher, an interpreter, a torch import and a process group per rank
// (profiles/r04/final/launch_cost.txt) -- against a 0.6-s fill at N = 5,000.  pc_multi_* does the same static shard with none of
// that: one pc_ctx per device, a host thread per device for the length of a call, every device uploaded in parallel, each filling
// the pairs of the target genomes it is dealt (the cost-balanced deal: deterministic, so every context arrives at the same
// partition by itself), and ONE exchange -- every device copies its shard to the root's gather buffer, device to device (peer
// copies: xGMI between the GPUs of a node) -- before the root permutes the shards into condensed order and delivers them to the
// host.  The reference spreads the same pair list over `cpus` worker processes (matrix.py:471-493).
// The fills that deliver no dense matrix (pc_multi_fill_edges / _components / _nearest / _tree / _between / _affinity, at the end of this file) deal contiguous
// stretches of targets instead, one per device, and merge the devices' small per-genome state on the root.
// ---------------------------------------------------------------------------------------------------------------------
struct pc_multi {
    std::vector<pc_ctx*> ctx;               // ctx[0] is the root: it holds the gather buffer, the assembled matrix and the pinned result
    DevBuf b_gather;                        // root device: world x stride doubles
    std::vector<DevBuf> b_shard;            // device r: its shard, stride doubles (allocated on that device)
    std::vector<int32_t> peer;              // device r -> root: PC_PEER_* (how its shard will travel), see pc_multi_peer_access
    std::vector<std::string> peer_note;     // the runtime's own words where access was refused
    bool uploaded = false, residues = false;
    // pc_multi_fill_edges / _components / _nearest / _tree
    DevBuf b_stage;                         // root device: the other devices' state (lists or forests), one slice per shipping device
    std::vector<int32_t> stretches;         // [world + 1] the deal of the last such call (pc_multi_last_stretches)
    float last_slab_ms[2] = {0.f, 0.f};     // ... its exchange and merge (pc_multi_last_slab_times)
};

namespace {
// fn(rank) on one host thread per device; the first failure (status, message) is re-raised on the calling thread
template <class F> int multi_each(pc_multi* m, F fn) {
    const int n = (int)m->ctx.size();
    std::vector<int> rc(n, PC_OK);
    std::vector<std::string> msg(n);
    auto work = [&](int r) { rc[r] = fn(r); if (rc[r] != PC_OK) msg[r] = pc_last_error(); };
    if (n == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int r = 0; r < n; ++r) th.emplace_back(work, r);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < n; ++r) if (rc[r] != PC_OK) { pc_set_error("device %d (rank %d of %d): %s", m->ctx[r]->device, r, n, msg[r].c_str()); return rc[r]; }
    return PC_OK;
}
}  // namespace

extern "C" int pc_multi_create(pc_multi** out, const int* device_ids, int n_dev) {
    if (!out) { pc_set_error("pc_multi_create: out is NULL"); return PC_ERR_ARG; }
    *out = nullptr;
    if (!device_ids || n_dev < 1 || n_dev > 64) { pc_set_error("pc_multi_create: %d devices", n_dev); return PC_ERR_ARG; }
    pc_multi* m = new (std::nothrow) pc_multi();
    if (!m) { pc_set_error("out of host memory"); return PC_ERR_ARG; }
    m->b_shard.resize((size_t)n_dev);
    for (int r = 0; r < n_dev; ++r) {
        pc_ctx* c = nullptr;
        const int rc = pc_ctx_create(&c, device_ids[r]);
        if (rc != PC_OK) { pc_multi_destroy(m); return rc; }
        m->ctx.push_back(c);
    }
    // peer access root <- every other device where the hardware offers it.  Without it the copies still work (the runtime stages
    // them through host memory), only slower: so a refusal is no error, but it is RECORDED per device (pc_multi_peer_access) --
    // a node whose exchange crawls must be able to say why.
    m->peer.assign((size_t)n_dev, PC_PEER_SAME_DEVICE);
    m->peer_note.assign((size_t)n_dev, std::string());
    for (int r = 1; r < n_dev; ++r) {
        if (m->ctx[r]->device == m->ctx[0]->device) continue;
        int can = 0;
        hipError_t e = hipDeviceCanAccessPeer(&can, m->ctx[r]->device, m->ctx[0]->device);
        if (e != hipSuccess) {
            m->peer[r] = PC_PEER_FAILED;
            m->peer_note[r] = std::string("hipDeviceCanAccessPeer: ") + hipGetErrorString(e);
            (void)hipGetLastError();
            continue;
        }
        if (!can) { m->peer[r] = PC_PEER_UNAVAILABLE; m->peer_note[r] = "hipDeviceCanAccessPeer says no: copies staged by the runtime"; continue; }
        PcDeviceGuard guard(m->ctx[r]->device);
        e = hipDeviceEnablePeerAccess(m->ctx[0]->device, 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) m->peer[r] = PC_PEER_ENABLED;
        else { m->peer[r] = PC_PEER_FAILED; m->peer_note[r] = std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e); }
        (void)hipGetLastError();
    }
    *out = m;
    return PC_OK;
}

extern "C" void pc_multi_destroy(pc_multi* m) {
    if (!m) return;
    for (size_t r = 0; r < m->ctx.size(); ++r) {           // (each device's buffers freed under its own guard, not by the destructors)
        if (!m->ctx[r]) continue;
        { PcDeviceGuard guard(m->ctx[r]->device); if (r < m->b_shard.size()) m->b_shard[r].release(); if (r == 0) { m->b_gather.release(); m->b_stage.release(); } }
        pc_ctx_destroy(m->ctx[r]);
    }
    delete m;
}

extern "C" int pc_multi_devices(const pc_multi* m) { return m ? (int)m->ctx.size() : -1; }

// How each device's shard reaches the root (decided once, in pc_multi_create): granted[r] = PC_PEER_*.  Returns the number of
// devices whose copies will NOT go device to device (PC_PEER_UNAVAILABLE / PC_PEER_FAILED); their reasons, one per line, are left
// for pc_last_error() -- as a note, not a failure: the call's status is that count (>= 0) or PC_ERR_ARG.
extern "C" int pc_multi_peer_access(const pc_multi* m, int32_t* granted) {
    if (!m) { pc_set_error("pc_multi_peer_access: NULL"); return PC_ERR_ARG; }
    int staged = 0;
    std::string note;
    for (size_t r = 0; r < m->ctx.size(); ++r) {
        if (granted) granted[r] = m->peer[r];
        if (m->peer[r] == PC_PEER_UNAVAILABLE || m->peer[r] == PC_PEER_FAILED) {
            ++staged;
            char line[256];
            snprintf(line, sizeof line, "device %d -> root %d: %s\n", m->ctx[r]->device, m->ctx[0]->device, m->peer_note[r].c_str());
            note += line;
        }
    }
    if (staged) pc_set_error("%s", note.c_str());
    return staged;
}

// Every device gets the same packed genomes (they are replicated: 0.2 GB at N = 5,000), in parallel.  with_residues = 0: part 1 only
// (all the set metrics need); an aai / peq fill uploads the residues on demand.
extern "C" int pc_multi_upload(pc_multi* m, const pc_packed* g, int with_residues) {
    if (!m || !g) { pc_set_error("pc_multi_upload: NULL argument"); return PC_ERR_ARG; }
    m->uploaded = false; m->residues = false;
    int rc = multi_each(m, [&](int r) { return with_residues ? pc_upload(m->ctx[r], g) : pc_upload_sets(m->ctx[r], g); });
    if (rc != PC_OK) return rc;
    m->uploaded = true; m->residues = with_residues != 0;
    return PC_OK;
}
extern "C" int pc_multi_upload_residues(pc_multi* m, const pc_packed* g) {
    if (!m || !g) { pc_set_error("pc_multi_upload_residues: NULL argument"); return PC_ERR_ARG; }
    if (!m->uploaded) { pc_set_error("pc_multi_upload_residues: pc_multi_upload first"); return PC_ERR_STATE; }
    int rc = multi_each(m, [&](int r) { return pc_upload_residues(m->ctx[r], g); });
    if (rc == PC_OK) m->residues = true;
    return rc;
}
extern "C" int pc_multi_set_tie_rule(pc_multi* m, int rule) {
    if (!m) { pc_set_error("pc_multi_set_tie_rule: NULL"); return PC_ERR_ARG; }
    for (pc_ctx* c : m->ctx) { const int rc = pc_set_tie_rule(c, rule); if (rc != PC_OK) return rc; }
    return PC_OK;
}

// The whole matrix over the devices of `m`: *out_host points to f64[N(N-1)/2] in page-locked memory the ROOT context owns (valid until
// the next fill or upload).  stats (optional, an array of pc_multi_devices() entries): every device's own fill.  exchange_ms /
// assemble_ms (optional): HIP-event times of the slowest device's copy to the root and of the root's permutation.
extern "C" int pc_multi_fill_borrow(pc_multi* m, int metric, int as_distance, const double** out_host, pc_stats* stats, float* exchange_ms, float* assemble_ms) {
    if (!m || !out_host) { pc_set_error("pc_multi_fill_borrow: NULL argument"); return PC_ERR_ARG; }
    *out_host = nullptr;
    if (!m->uploaded) { pc_set_error("pc_multi_fill_borrow: pc_multi_upload first"); return PC_ERR_STATE; }
    const int world = (int)m->ctx.size();
    pc_ctx* root = m->ctx[0];
    if (world == 1) {
        if (exchange_ms) *exchange_ms = 0.f;
        if (assemble_ms) *assemble_ms = 0.f;
        return pc_fill_borrow(root, metric, as_distance, out_host, stats);
    }
    const int N = root->dev.N;
    const int64_t np = (int64_t)N * (N - 1) / 2;
    // 1 the deal (every context computes the same one), shard buffers
    int rc = multi_each(m, [&](int r) -> int {
        pc_ctx* c = m->ctx[r];
        int e = pc_set_shard_balanced(c, r, world);
        if (e != PC_OK) return e;
        PcDeviceGuard guard(c->device);
        return abi_rc(m->b_shard[r].ensure((size_t)std::max<int64_t>(c->shard_stride, 1) * 8));
    });
    if (rc != PC_OK) return rc;
    const int64_t stride = root->shard_stride;
    for (pc_ctx* c : m->ctx) if (c->shard_stride != stride) { pc_set_error("pc_multi_fill_borrow: the devices disagree on the deal (stride %lld vs %lld)", (long long)c->shard_stride, (long long)stride); return PC_ERR_STATE; }
    {
        PcDeviceGuard guard(root->device);
        const size_t bytes = (size_t)std::max<int64_t>(np, 1) * 8;
        if ((rc = abi_rc(m->b_gather.ensure((size_t)std::max<int64_t>(stride, 1) * 8 * (size_t)world))) ||
            (rc = abi_rc(root->b_out.ensure(bytes))) || (rc = root->h_out.ensure(bytes))) return rc;
    }
    // 2 every device fills its shard, then copies it to its slice of the root's gather buffer: the one exchange
    std::vector<float> xms((size_t)world, 0.f);
    std::vector<pc_stats> local((size_t)world);
    rc = multi_each(m, [&](int r) -> int {
        pc_ctx* c = m->ctx[r];
        int e = pc_fill_shard_dev(c, metric, as_distance, m->b_shard[r].p, c->stream, &local[r]);       // (with stats: returns when the fill is done)
        if (e != PC_OK) return e;
        PcDeviceGuard guard(c->device);
        PC_HIP(hipEventRecord(c->ev[0], c->stream));
        double* dst = m->b_gather.as<double>() + (size_t)r * (size_t)stride;
        if (c->device == root->device) PC_HIP(hipMemcpyAsync(dst, m->b_shard[r].p, (size_t)stride * 8, hipMemcpyDeviceToDevice, c->stream));
        else PC_HIP(hipMemcpyPeerAsync(dst, root->device, m->b_shard[r].p, c->device, (size_t)stride * 8, c->stream));
        PC_HIP(hipEventRecord(c->ev[1], c->stream));
        PC_HIP(hipStreamSynchronize(c->stream));
        PC_HIP(hipEventElapsedTime(&xms[r], c->ev[0], c->ev[1]));
        return (int)PC_OK;
    });
    if (rc != PC_OK) return rc;
    // 3 the root permutes the shards into condensed order and delivers
    {
        PcDeviceGuard guard(root->device);
        PC_HIP(hipEventRecord(root->ev[0], root->stream));
        if ((rc = pc_assemble_dev(root, m->b_gather.p, world, root->b_out.p, root->stream))) return rc;
        PC_HIP(hipEventRecord(root->ev[1], root->stream));
        if (np) PC_HIP(hipMemcpyAsync(root->h_out.p, root->b_out.p, (size_t)np * 8, hipMemcpyDeviceToHost, root->stream));
        PC_HIP(hipStreamSynchronize(root->stream));
        if (assemble_ms) PC_HIP(hipEventElapsedTime(assemble_ms, root->ev[0], root->ev[1]));
    }
    if (exchange_ms) *exchange_ms = *std::max_element(xms.begin(), xms.end());
    if (stats) for (int r = 0; r < world; ++r) stats[r] = local[r];
    *out_host = root->h_out.as<double>();
    return PC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Edge, component, nearest, tree, between-groups, affinity and distribution fills over the devices of a pc_multi: one driver, multi_slab_fill<Fill>, over the fill's description
// (pc_host.h, pc_fill_slabs.hip).  Each device runs the description's begin and the walk over ONE contiguous stretch of targets with
// the call's state on its own device, and ships that state to the root; the state merges exactly -- lists by their total order,
// forests by uniting g with its foreign parent, edge lists over ascending stretches by concatenation -- so the root's end delivers
// what one context would have.  See the header for the deal and for what travels.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// Ahead of the devices' work: the refusals, every context unsharded, and the deal.  Returns PC_OK with `single` set when the root alone
// serves the call (one device, or no pair to fill).
int slab_prepare(pc_multi* m, PcSlabRun& run, const char* what, bool& single) {
    int rc = PC_OK;
    single = false;
    if (!m) { pc_set_error("%s: NULL argument", run.who); return PC_ERR_ARG; }
    if (!m->uploaded) { pc_set_error("%s: pc_multi_upload first", run.who); return PC_ERR_STATE; }
    const int world = (int)m->ctx.size();
    for (pc_ctx* c : m->ctx) if (c->world != 1 && (rc = pc_set_shard(c, 0, 1))) return rc;     // (a dense pc_multi_fill_borrow leaves its deal in force)
    pc_ctx* root = m->ctx[0];
    const int N = root->dev.N;
    m->last_slab_ms[0] = m->last_slab_ms[1] = 0.f;
    m->stretches.assign((size_t)world + 1, 0);
    m->stretches[world] = N;
    if (world == 1 || N <= 1) { for (int r = 1; r < world; ++r) m->stretches[r] = N; single = true; return PC_OK; }
    if ((rc = pc_slab_check(root, run, what))) return rc;
    // the deal: contiguous stretches of about equal cost, computed once, on the root
    std::vector<uint64_t> cost((size_t)N);
    if (run.metric >= PC_AAI) {
        PcDeviceGuard guard(root->device);
        if (!guard.ok) return PC_ERR_HIP;
        if ((rc = wait_last_work(root, nullptr, false))) return rc;
        PC_HIP(hipStreamSynchronize(root->stream));
        if ((rc = pc_count_target_costs(root))) return rc;
        for (int t = 0; t < N; ++t) cost[t] = root->target_cost[t] + (uint64_t)t * 2000u;
    } else {
        for (int t = 0; t < N; ++t) cost[t] = (uint64_t)t;
    }
    return pc_stretch_plan(cost.data(), N, world, m->stretches.data());
}

// The call `run` over the devices of m; on PC_OK the run holds the results and the stats of the root (pc_slab_call delivers them, the
// stats as stats[0]) and stats[r], when asked for, the fills of device r > 0.
template <class Fill> int multi_slab_fill(pc_multi* m, PcSlabRun& run, pc_stats* stats) {
    int rc = PC_OK;
    bool single = false;
    if ((rc = slab_prepare(m, run, Fill::what, single))) return rc;
    const int world = (int)m->ctx.size();
    pc_ctx* root = m->ctx[0];
    if (single) {                                                           // the single-context call, under its own name
        if (stats) for (int r = 1; r < world; ++r) memset(&stats[r], 0, sizeof(pc_stats));
        run.who = Fill::who;
        return pc_slab_fill<Fill>(root, run);
    }
    PcRange range(Fill::multi_range);
    // a slice of the root's staging buffer for every device that ships: the non-root devices with a stretch, in rank order
    std::vector<int> slot((size_t)world, -1);
    int n_foreign = 0;
    for (int r = 1; r < world; ++r) if (m->stretches[r] < m->stretches[r + 1]) slot[r] = n_foreign++;
    const size_t bytes = Fill::ship_bytes(root, run);
    if (bytes) {
        PcDeviceGuard guard(root->device);
        if (!guard.ok) return PC_ERR_HIP;
        if ((rc = abi_rc(m->b_stage.ensure(std::max<size_t>((size_t)n_foreign * bytes, 16))))) return rc;
    }
    std::vector<PcSlabRun> runs((size_t)world, run);
    std::vector<float> xms((size_t)world, 0.f);
    rc = multi_each(m, [&](int r) -> int {
        pc_ctx* c = m->ctx[r];
        const int ta = m->stretches[r], tb = m->stretches[r + 1];
        if (r != 0 && ta == tb) return (int)PC_OK;                          // an empty stretch: nothing launched, nothing shipped
        PcDeviceGuard guard(c->device);
        if (!guard.ok) return (int)PC_ERR_HIP;
        int e = PC_OK;
        if ((e = Fill::begin(c, runs[r])) || (e = pc_slab_stretch<Fill>(c, runs[r], ta, tb))) return e;
        if (r == 0 || !bytes) return (int)PC_OK;
        // the one exchange: this device's state into its slice on the root, timed between its events 0 and 1
        if ((e = Fill::ship(c, root, runs[r], m->b_stage.p, slot[r], n_foreign))) return e;
        PC_HIP(hipStreamSynchronize(c->stream));
        c->busy = false;
        PC_HIP(hipEventElapsedTime(&xms[r], c->ev[0], c->ev[1]));
        return (int)PC_OK;
    });
    if (rc != PC_OK) return rc;
    int64_t slabs = 0;
    for (const PcSlabRun& one : runs) slabs += one.n_slabs;
    m->last_slab_ms[0] = *std::max_element(xms.begin(), xms.end());
    {
        // the merge on the root (the copies have arrived: every shipping stream was drained), between the root's events 0 and 1 where it
        // is a launch, then the root's own end
        PcDeviceGuard guard(root->device);
        if (!guard.ok) return PC_ERR_HIP;
        if ((rc = Fill::merge(m->ctx, runs, m->b_stage.p, n_foreign, &m->last_slab_ms[0])) || (rc = Fill::end(root, runs[0]))) return rc;
        if (bytes) PC_HIP(hipEventElapsedTime(&m->last_slab_ms[1], root->ev[0], root->ev[1]));
    }
    run = runs[0];
    run.n_slabs = (int32_t)slabs;
    if (stats) for (int r = 1; r < world; ++r) stats[r] = runs[r].sum;
    return PC_OK;
}
}  // namespace

extern "C" int pc_multi_fill_edges(pc_multi* m, int metric, int as_distance, double threshold, int64_t slab_bytes,
                                   const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_edges"; run.metric = metric; run.as_distance = as_distance; run.threshold = threshold; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcEdgesFill>(run, {src, tgt, val, n_edges, n_slabs}, stats, [&] { return multi_slab_fill<PcEdgesFill>(m, run, stats); });
}

extern "C" int pc_multi_fill_components(pc_multi* m, int metric, int as_distance, double threshold, int strict, int64_t slab_bytes,
                                        const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_components"; run.metric = metric; run.as_distance = as_distance; run.strict = strict; run.threshold = threshold;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcComponentsFill>(run, {labels, n_components, n_edges, n_slabs}, stats, [&] { return multi_slab_fill<PcComponentsFill>(m, run, stats); });
}

extern "C" int pc_multi_fill_nearest(pc_multi* m, int metric, int as_distance, int k, int64_t slab_bytes,
                                     const int32_t** nbr, const double** val, int32_t* k_out, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_nearest"; run.metric = metric; run.as_distance = as_distance; run.k = k; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcNearestFill>(run, {nbr, val, k_out, n_slabs}, stats, [&] { return multi_slab_fill<PcNearestFill>(m, run, stats); });
}

extern "C" int pc_multi_fill_tree(pc_multi* m, int metric, int as_distance, int64_t slab_bytes,
                                  const int32_t** src, const int32_t** tgt, const double** val, int32_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_tree"; run.metric = metric; run.as_distance = as_distance; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcTreeFill>(run, {src, tgt, val, n_edges, n_slabs}, stats, [&] { return multi_slab_fill<PcTreeFill>(m, run, stats); });
}

extern "C" int pc_multi_fill_between(pc_multi* m, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                                     const int64_t** sum, const int64_t** count, const int32_t** lo, const int32_t** hi, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_between"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcBetweenFill>(run, {sum, count, lo, hi, n_slabs}, stats, [&] { return multi_slab_fill<PcBetweenFill>(m, run, stats); });
}

extern "C" int pc_multi_fill_affinity(pc_multi* m, int metric, int as_distance, const int32_t* group, int n_groups, int want_table, int64_t slab_bytes,
                                      const int64_t** own_sum, const int32_t** own_lo, const int32_t** own_hi, const int32_t** near_group,
                                      const int64_t** near_sum, const int32_t** near_lo, const int32_t** near_hi,
                                      const int64_t** tab_sum, const int32_t** tab_lo, const int32_t** tab_hi, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_affinity"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.want_table = want_table != 0; run.slab_bytes = slab_bytes;
    return pc_slab_call<PcAffinityFill>(run, {own_sum, own_lo, own_hi, near_group, near_sum, near_lo, near_hi, tab_sum, tab_lo, tab_hi, n_slabs}, stats,
                                        [&] { return multi_slab_fill<PcAffinityFill>(m, run, stats); });
}

extern "C" int pc_multi_fill_hist(pc_multi* m, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                                  const int64_t** hist, int32_t* n_classes, int64_t* n_pairs, int32_t* n_slabs, pc_stats* stats) {
    PcSlabRun run; run.who = "pc_multi_fill_hist"; run.metric = metric; run.as_distance = 1; run.bt_invert = !as_distance; run.group = group; run.n_groups = n_groups;
    run.slab_bytes = slab_bytes;
    return pc_slab_call<PcHistFill>(run, {hist, n_classes, n_pairs, n_slabs}, stats, [&] { return multi_slab_fill<PcHistFill>(m, run, stats); });
}

extern "C" int pc_multi_last_stretches(const pc_multi* m, int32_t* bounds) {
    if (!m || !bounds) { pc_set_error("pc_multi_last_stretches: NULL argument"); return PC_ERR_ARG; }
    if (m->stretches.size() != m->ctx.size() + 1) { pc_set_error("pc_multi_last_stretches: no edge, component, nearest or tree fill has run on these devices"); return PC_ERR_STATE; }
    memcpy(bounds, m->stretches.data(), m->stretches.size() * sizeof(int32_t));
    return PC_OK;
}

extern "C" int pc_multi_last_slab_times(const pc_multi* m, float* ms_exchange, float* ms_merge) {
    if (!m) { pc_set_error("pc_multi_last_slab_times: NULL"); return PC_ERR_ARG; }
    if (ms_exchange) *ms_exchange = m->last_slab_ms[0];
    if (ms_merge) *ms_merge = m->last_slab_ms[1];
    return PC_OK;
}
