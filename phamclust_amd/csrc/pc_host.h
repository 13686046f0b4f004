// pc_host.h -- internal header of the host units of libphamclust_hip.so (pc_ctx, pc_upload, pc_align, pc_fill, pc_fill_slabs, pc_multi.hip):
// the context, its buffers and the helpers they share.  Not installed, not part of the C-ABI.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pc_common.h"
#include "pc_nw_geometry.h"
#include "../../include/phamclust_hip.h"

// roctx range around a stage of a fill (the marker library is looked up in pc_ctx.hip)
struct PcRange {
    bool on;
    explicit PcRange(const char* name);
    ~PcRange();
    PcRange(const PcRange&) = delete; PcRange& operator=(const PcRange&) = delete;
};

// internal status: a device allocation failed.  A chunked fill answers it with smaller chunks; at the C-ABI it is PC_ERR_HIP.
constexpr int PC_ERR_NOMEM_INTERNAL = -100;
// marks the planning stage of a fill: the test-hooks build refuses device allocations above PC_FAKE_OOM_ABOVE inside it (pc_ctx.hip)
struct PlanningScope { PlanningScope(); ~PlanningScope(); };
// the value triangle pc_hook_slab_values set (target-major, *n_pairs doubles), or NULL: always NULL in the release library (pc_ctx.hip).
// slab_walk overwrites every slab it has filled with its part of the triangle.  (Not part of the exported set.)
__attribute__((visibility("hidden"))) const double* pc_hooked_slab_values(int64_t* n_pairs);
// the rows pc_hook_rows_values set (f64[*n_rows][*n], row k for the call's rows[k]), or NULL: always NULL in the release library.
// rows_walk overwrites every rows slab it has filled with its rows of them.  (Not part of the exported set.)
__attribute__((visibility("hidden"))) const double* pc_hooked_rows_values(int32_t* n_rows, int32_t* n);
// Grow-only device buffer that owns its memory: freed when it goes out of scope, on whichever device is current then (the
// context's destruction runs under its device guard).  Move-only, so that a std::vector of them can grow.
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~DevBuf() { release(); }
    int ensure(size_t bytes);
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};
// Grow-only page-locked host buffer: ensure(bytes) frees the old buffer first, then allocates bytes + bytes / 8.
struct PinnedBuf {
    void* p = nullptr; size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int ensure(size_t bytes);
    int grow_keep(size_t bytes, size_t used);   // as ensure, but the first `used` bytes survive a growth (new buffer, copy, free)
    template <class T> T* as() const { return (T*)p; }
};

// fn(begin, end) over [0, n) on up to 16 host threads (upload-time indexing of ~10^8 residues)
template <class F> void parallel_chunks(int64_t n, F fn, int64_t grain = 4096) {
    int nt = (int)std::min<int64_t>(std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u), (n + grain - 1) / grain);
    if (nt <= 1) { fn((int64_t)0, n); return; }
    std::vector<std::thread> th;
    const int64_t per = (n + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) th.emplace_back([=] { fn(std::min(n, t * per), std::min(n, (t + 1) * per)); });
    for (auto& x : th) x.join();
}

static inline int abi_rc(int rc) { return rc == PC_ERR_NOMEM_INTERNAL ? PC_ERR_HIP : rc; }

static int upload_raw(DevBuf& b, const void* p, size_t bytes) {
    int rc = abi_rc(b.ensure(std::max<size_t>(bytes, 16)));
    if (rc != PC_OK) return rc;
    if (bytes) PC_HIP(hipMemcpy(b.p, p, bytes, hipMemcpyHostToDevice));
    return PC_OK;
}

template <class T> int upload_vec(DevBuf& b, const std::vector<T>& v) {
    int rc = abi_rc(b.ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (rc != PC_OK) return rc;
    if (!v.empty()) PC_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return PC_OK;
}

struct pc_ctx {
    int device = 0;
    int n_cu = 256;                         // compute units of THIS context's device (grid sizing of the persistent tile kernels)
    hipStream_t stream = nullptr;
    bool uploaded = false;                  // part 1 of the upload is on the device (set metrics can run)
    bool residues_ready = false;            // ... and part 2 (aai / peq, pc_align_pairs can run)
    int64_t n_residue_bytes_in = 0;         // residue bytes of the packed genomes part 1 saw (part 2 must be given the same)
    PcDev dev{};
    std::vector<int32_t> h_gene_len;
    std::vector<uint32_t> h_sp_n;                      // [N] a genome's entries of phams with at least two holders (k_sparse_col's pocp / af modes: values per block of targets)
    int max_ent_len = 0;                               // largest summed length of a (genome, pham) entry (k_sparse_col's af mode keeps them as 16-bit values)
    std::vector<uint8_t> h_gene_odd;                   // gene holds a byte outside the 24-letter alphabet
    int max_gene_len = 0, min_gene_len = 0, max_nph = 0, max_ngen = 0;
    int64_t max_tlen = 0;                    // largest summed translation length of a genome
    double avg_shared = 0.0;                 // phams an average genome pair shares (pocp's kernel choice)
    int two_holder = 0;                      // phams at least two genomes hold (dev.sp_W = their 64-id words)
    // kernel-variant classes over column genes
    int ncls_all = 0;                       // BASE classes: variant * 4 + lanes-per-segment bucket (twice: "any byte" columns), last = general kernel
    int nlc = 0;                            // launch classes = ncls_all * PC_WAVE_MODES (base class x workgroup shape of the task, pc_common.h)
    std::vector<int32_t> cls_max_lb;        // [nlc] longest column sequence that can land in the launch class (LDS size of its launch)
    PcTaskPlan task_plan{};
    // shard
    int rank = 0, world = 1;
    int64_t shard_pairs = 0, shard_stride = 0;
    PcShard shard{};
    bool balanced = false;                  // cost-balanced deal in force (pc_set_shard_balanced): assembly goes through the tables
    std::vector<uint64_t> target_cost;      // DP cells per target genome, computed once per upload
    std::vector<int32_t> h_t_rank;          // the deal in force, host copy: owner rank of each target genome ...
    std::vector<int64_t> h_t_lbase;         // ... and where its pairs start inside that rank's shard
    std::vector<int32_t> h_owned;           // this rank's targets, ascending, and
    std::vector<int64_t> h_lbase;           // [nown+1] the shard-local index of pair (0, owned[k]) (host copies of shard.owned / lbase)
    // persistent device arrays
    DevBuf b_raw, b_seq_tmp;                // part 2's staging: the raw residue bytes and their offsets, as uploaded (encoded into b_codes on the device)
    DevBuf b_sets;                          // part 1 of the upload, one allocation: bitmap | rank table | gene lengths | entry offsets | nph | ngen | tlen | 4 entry arrays
    PinnedBuf h_stage;                      // its page-locked host image
    PinnedBuf h_raw;                        // page-locked staging of the raw residues (part 2; <= 512 MB)
    DevBuf b_gene_off, b_codes;
    DevBuf b_gene_q, b_q_gene, b_q_class, b_q_nseg, b_rem_class, b_cls_begin, b_task_rows, b_owned, b_lbase, b_t_rank, b_t_lbase, b_cost;
    // work buffers (grow-only)
    DevBuf b_na, b_off, b_key0, b_key1, b_val0, b_val1, b_sort_tmp, b_flags, b_excl, b_alias, b_start_q, b_end_q, b_ntask_q, b_task_off_q, b_scan_tmp;
    DevBuf b_tasks, b_tasks_sorted, b_bucket_row, b_bucket_dest, b_res, b_totals, b_plan, b_scratch, b_out, b_lut, b_slice_begin, b_aln_t;
    DevBuf b_rows, b_row_of;                // the domain of the last rows fill (PcRows: the query genomes, and every genome's position among them)
    DevBuf b_grp_genome, b_grp_end, b_grp_rowbase, b_grp_trow, b_grp_tcol;   // the domain of the last groups fill (PcGroups)
    DevBuf b_pr_src, b_pr_tgt, b_pr_at;     // the domain of the last pair-list fill (PcPairs): the caller's list as uploaded, then sorted
    // pc_fill_edges: the resident slab (shard layout) and its shard tables, chunk counts / offsets, one slab's edges
    DevBuf b_edge_slab, b_edge_owned, b_edge_lbase, b_edge_cnt, b_edge_off, b_edge_src, b_edge_tgt, b_edge_val;
    DevBuf b_edge_bars;                     // pc_fill_edges_bars: bar[N], resident for the call
    DevBuf b_rq_rows, b_rq_query;           // a rows slab fill: every query row of the call, ascending, and is_query[N] (PcRowsSlab)
    PinnedBuf h_edge_src, h_edge_tgt, h_edge_val;   // the edge list lent out by pc_fill_edges (grown by copying: pinned_grow_keep)
    hipEvent_t ev_slab[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // the passes over a slab, of whichever of the three fills runs: created by the first one that is asked for stats
    float last_edge_ms[2] = {0.f, 0.f};     // count + scan + emit, edges' D2H of the last pc_fill_edges with stats (pc_last_edge_times)
    // pc_fill_components: parent[N], labels[N] + the 8-byte count of passing pairs behind them (one D2H), and their pinned host image
    DevBuf b_cc_parent, b_cc_labels;
    PinnedBuf h_cc_labels;                  // the labels lent out by pc_fill_components
    float last_cc_ms[2] = {0.f, 0.f};       // union passes, labels pass of the last pc_fill_components with stats (pc_last_component_times)
    // pc_fill_nearest: key[N][K] (order-preserving u64 of the value), then val[N][K] | nbr[N][K] (one D2H), and their pinned host image
    DevBuf b_nn_key, b_nn_out;
    DevBuf b_np_val, b_np_start;            // pc_nearest_of_pairs: the caller's val[L]; start[N + 1] of the owners' runs (its result: val[N][kk] | nbr[N][kk] | count[N] in b_nn_out / h_nn)
    PinnedBuf h_nn;                         // the neighbours and values lent out by pc_fill_nearest
    float last_nn_ms[2] = {0.f, 0.f};       // row + column passes, finishing pass of the last pc_fill_nearest / pc_fill_rows_nearest with stats (pc_last_nearest_times)
    // pc_fill_tree: comp[N] | next[N], best[N], two lists of N + PC_TREE_TAIL keys (the resident forest and the one a pass writes), the
    // rounds' live words; the keys' pinned host image and the pinned result val[N] | src[N] | tgt[N]
    DevBuf b_tree_comp, b_tree_best, b_tree_list, b_tree_live;
    PinnedBuf h_tree_keys, h_tree;          // the edges lent out by pc_fill_tree
    int tree_cur = 0;                       // which of the two lists is the resident forest
    float last_tree_ms[2] = {0.f, 0.f};     // rounds (with stats), finish of the last pc_fill_tree (pc_last_tree_times)
    int32_t last_tree_rounds[2] = {0, 0};   // ... its rounds that did work, and those enqueued (pc_last_tree_rounds)
    // pc_fill_between: group[N], the resident accumulator and the folded table (pc_between_bytes(G) each: pc_common.h), the table's pinned host image
    DevBuf b_bt_group, b_bt_acc, b_bt_out;
    PinnedBuf h_bt;                         // the four arrays lent out by pc_fill_between
    float last_bt_ms[2] = {0.f, 0.f};       // passes, fold of the last pc_fill_between / pc_fill_rows_between with stats (pc_last_between_times)
    // pc_fill_affinity: group[N], member[N] (the genomes sorted by (group, index)), goff[G + 1], the column pass's group ranges, the resident
    // table (pc_affinity_table_bytes) and the result (pc_affinity_out_bytes: pc_common.h), the result's pinned host image
    // pc_fill_rows_affinity: the same buffers -- group[N] (-1: in no group), goff over the labelled genomes, the resident state in b_af_tab
    // (pc_affinity_rows_state_bytes), the result in b_af_out / h_af (pc_affinity_rows_out_bytes) -- and qcount[G], the query genomes of each group
    DevBuf b_af_group, b_af_member, b_af_goff, b_af_range, b_af_tab, b_af_out, b_af_qcount;
    PinnedBuf h_af;                         // the arrays lent out by pc_fill_affinity
    int af_ranges = 0;                      // group ranges of the column pass (b_af_range holds af_ranges + 1 bounds)
    float last_af_ms[3] = {0.f, 0.f, 0.f};  // row passes, finish, column passes of the last pc_fill_affinity / pc_fill_rows_affinity with stats (pc_last_affinity_times)
    // pc_fill_hist: group[N] (a partition only), the resident state and the finished result (pc_hist_bytes(classes) each: pc_common.h), the
    // result's pinned host image
    DevBuf b_hist_group, b_hist_state, b_hist_out;
    PinnedBuf h_hist;                       // the histogram lent out by pc_fill_hist
    float last_hist_ms[2] = {0.f, 0.f};     // passes, finish of the last pc_fill_hist / pc_fill_rows_hist with stats (pc_last_hist_times)
    PinnedBuf h_plan;                       // u32 [ncls+1] task offsets, then from word 1000 the u64 totals
    // what the last alignment plan (stage_plan) left in the work buffers, for the stages that follow it
    struct PlanState {
        bool valid = false; int ppos = 0; int condensed = 1; int64_t A = 0, n_distinct = 0; uint32_t ntasks = 0;
        int k0 = 0, k1 = 0;                 // the owned targets [k0, k1) the plan covers (a chunk of the shard, or all of it)
        bool whole = false;                 // ... all of an unsharded context: what the alignment-sliced route needs
        std::vector<uint32_t> tb;           // [ncls+1] task range per launch class in b_tasks_sorted
        pc_stats st;                        // counts of the plan (alignments, cells, tasks, distinct ...)
    } plan;
    // tasks per launch class: what the last stage_align launched (all of a plan's tasks, or one slice of them) ...
    std::vector<uint32_t> aligned_tasks;    // [nlc]
    // ... and what pc_last_plan_tasks reports: the sum over the chunks of the last aai / peq fill; after pc_plan_dev the whole
    // plan's counts, after pc_align_slice_dev that slice's
    std::vector<int64_t> last_plan_tasks;   // [nlc]
    bool last_plan_tasks_valid = false;
    PinnedBuf h_out;                        // result buffer lent out by pc_fill_borrow
    float last_align_ms = 0.f;              // kernel time of the last pc_align_pairs call
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    static constexpr int kAux = 15;         // + the caller's stream = up to 16 concurrent alignment launches (8 by default)
    hipStream_t aux[kAux] = {};             // alignment launches of different classes overlap on these
    hipEvent_t aux_ev[kAux + 1] = {};
    int n_streams = 8;                      // streams actually used (tuning knob: env PC_ALIGN_STREAMS at ctx creation)
    // Streams for the few launches whose TASKS run for tens of milliseconds (strip-mined passes over long genes).  Their own, so
    // that no other launch queues up behind them -- the runtime lays streams over a handful of hardware queues, and a queue runs
    // its launches one after the other: behind a 30-ms strip launch sat a dozen launches of a millisecond each -- and of HIGH
    // priority: those streams get hardware queues of their own, and their waves go first where they compete (they are the
    // fill's critical path).  PC_LONG_PRIORITY=0: ordinary priority.
    static constexpr int kLong = 4;
    hipStream_t lng[kLong] = {};
    hipEvent_t lng_ev[kLong] = {};
    int tie_rule = 0;                       // row of the aligner's tie-rule table (pc_set_tie_rule)
    int64_t lut_key = -1; const double* lut_ptr = nullptr;   // what the gcs / jc epilogue table in b_lut was built for
    hipEvent_t ev_last = nullptr;           // recorded at the end of every entry point that leaves work on a caller's stream
    bool busy = false;                      // ev_last was recorded and not waited for yet
    hipStream_t last_stream = nullptr;      // ... on this stream
    int last_set_kernel = -1;               // kernel family the last gcs / jc / pocp / af fill ran on (pc_last_set_kernel)
    pc_set_inputs last_set_inputs{};        // ... what the selector read for it and the shape its launcher took (pc_last_set_launch)
    pc_set_shape last_set_shape{};
    int64_t plan_budget = 0;                // bytes of plan buffers one chunk of an aai / peq fill may use; 0: automatic (pc_set_plan_budget)
};

// Every entry point runs on the context's device and leaves the calling thread's current device as it found it
// (PyTorch and other libraries in the process keep their own idea of "current device").
struct PcDeviceGuard {
    int prev = -1, dev = -1; bool ok = true;
    explicit PcDeviceGuard(int device) : dev(device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) {
            hipError_t e = hipSetDevice(dev);
            if (e != hipSuccess) { pc_set_error("hipSetDevice(%d): %s", dev, hipGetErrorString(e)); ok = false; }
        }
    }
    ~PcDeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
    PcDeviceGuard(const PcDeviceGuard&) = delete;
    PcDeviceGuard& operator=(const PcDeviceGuard&) = delete;
};
#define PC_ON_DEVICE(c) PcDeviceGuard pc_guard_((c)->device); if (!pc_guard_.ok) return PC_ERR_HIP

// A fill (or plan, slice, reduce) without stats returns while its kernels still run on the CALLER's stream and still use
// the context's work buffers and shard tables.  Every such entry point ends in mark_work(): ONE event, recorded after its
// last launch.  Anything that rewrites those buffers (upload, re-shard, the test hooks, work on another stream) first
// waits for it.
static int wait_last_work(pc_ctx* c, hipStream_t next_stream, bool same_stream_is_ordered) {
    if (!c->busy) return PC_OK;
    if (same_stream_is_ordered && next_stream == c->last_stream) return PC_OK;
    PC_HIP(hipEventSynchronize(c->ev_last));
    c->busy = false;
    return PC_OK;
}
static int mark_work(pc_ctx* c, hipStream_t st) {
    PC_HIP(hipEventRecord(c->ev_last, st));
    c->busy = true; c->last_stream = st;
    return PC_OK;
}

// A groups fill's domain as the host sees it: the device view, and per row block of TS positions where its tiles and its slots
// begin (both ascend: a range of row blocks is a range of the tile list and of the slots).
struct PcGroupsHost {
    PcGroups dev{};
    int nblocks = 0;                        // row blocks = ceil(M / TS)
    std::vector<int64_t> block_tile;        // [nblocks+1] first tile of row block a; [nblocks] = T
    std::vector<int64_t> block_slot;        // [nblocks+1] first slot of row block a = pos_rowbase[a * TS]; [nblocks] = L
};

// A pair-list fill's domain as the host sees it: the device view and its blocks of PC_PAIR_BLOCK slots.
struct PcPairsHost {
    PcPairs dev{};
    int nblocks = 0;                        // ceil(L / PC_PAIR_BLOCK); block k holds the slots [k * PC_PAIR_BLOCK, min((k + 1) * PC_PAIR_BLOCK, L))
};
// The domain of a fill that is cut into UNITS (fill_units): exactly one of the three is set -- the query rows of a rows fill, the row
// blocks of a groups fill, the blocks of slots of a pair-list fill.  None set: the owned targets of the context's shard (a whole fill).
struct PcUnitDomain {
    const PcRows* rows = nullptr;
    const PcGroupsHost* groups = nullptr;
    const PcPairsHost* pairs = nullptr;
    bool any() const { return rows || groups || pairs; }
    int units() const { return rows ? rows->nrows : groups ? groups->nblocks : pairs ? pairs->nblocks : 0; }
    int64_t slots(int k0, int k1, int N) const {              // a range of units is a range of slots
        if (rows) return (int64_t)(k1 - k0) * N;
        if (groups) return groups->block_slot[k1] - groups->block_slot[k0];
        return std::min<int64_t>((int64_t)k1 * PC_PAIR_BLOCK, pairs->dev.L) - (int64_t)k0 * PC_PAIR_BLOCK;
    }
};

// What every fill entry point checks of its context and its metric before anything of its own.  `who` names the caller in the message
// texts; `kind` != NULL ("a rows fill"): the call takes an unsharded context only.  ppos != NULL: PC_AAI_PPOS is folded into PC_AAI + *ppos.
static int fill_check(const pc_ctx* c, const char* who, const char* kind, int* metric, int* ppos) {
    if (!c || !c->uploaded) { pc_set_error("%s: upload first", who); return PC_ERR_STATE; }
    if (kind && c->world != 1) { pc_set_error("%s: context is sharded (%d/%d); %s is a one-GPU call on an unsharded context", who, c->rank, c->world, kind); return PC_ERR_STATE; }
    if (*metric < PC_GCS || *metric > PC_AAI_PPOS) { pc_set_error("%s: metric %d", who, *metric); return PC_ERR_ARG; }
    if (ppos && (*ppos = *metric == PC_AAI_PPOS)) *metric = PC_AAI;
    return PC_OK;
}
// ... and, once the call is known to have pairs to fill: aai / peq align residues
static int fill_check_residues(const pc_ctx* c, const char* who, int metric) {
    if (metric < PC_AAI || c->residues_ready) return PC_OK;
    pc_set_error("%s: aai / peq need the residues on the device (pc_upload, or pc_upload_residues after pc_upload_sets)", who);
    return PC_ERR_STATE;
}

// sum += one, field by field (the fills of a slab walk)
static void pc_stats_add(pc_stats& sum, const pc_stats& one) {
    sum.n_pairs += one.n_pairs; sum.n_alignments += one.n_alignments; sum.n_cells += one.n_cells; sum.n_tasks += one.n_tasks;
    sum.n_residue_bytes += one.n_residue_bytes; sum.n_align_launches += one.n_align_launches; sum.n_chunks += one.n_chunks;
    sum.ms_total += one.ms_total; sum.ms_plan += one.ms_plan; sum.ms_align += one.ms_align; sum.ms_reduce += one.ms_reduce;
    sum.n_distinct_alignments += one.n_distinct_alignments; sum.n_distinct_cells += one.n_distinct_cells;
}

// A slab fill (pc_fill_edges / pc_fill_components / pc_fill_nearest / pc_fill_tree / pc_fill_between / pc_fill_affinity / pc_fill_hist, and pc_multi_fill_* over several devices) is ONE description of the
// fill -- a struct of static functions, declared here and defined in pc_fill_slabs.hip (the launchers of its kernels live in pc_edges.hip,
// pc_components.hip, pc_nearest.hip, pc_tree.hip, pc_between.hip, pc_affinity.hip and pc_hist.hip) -- handed as a template argument to the drivers:
//   pc_slab_fill<Fill>      one context: check -> begin -> walk [0, N) -> end
//   pc_slab_stretch<Fill>   the walk over the targets [ta, tb): the slab cut, each slab filled and handed to Fill::slab
//   multi_slab_fill<Fill>   (pc_multi.hip) begin -> walk(its stretch) -> ship on every device, then merge -> end on the root
//   pc_rows_slab_fill<Fill> (pc_fill_slabs.hip) a rows form: check -> rows -> Seed::pack -> begin -> Seed::install -> walk the query rows -> end
// and every extern "C" entry point is its signature, the fields of the run that are its own, and pc_slab_call<Fill> around one of them.
// What a description says:
//   kind, Out   its PcSlabKind, and its output shape: the caller's output pointers (PcEdgeOut / PcLabelOut / PcListOut / PcTableOut / PcGenomeTableOut / PcHistOut), which can be
//           cleared, say whether all are there, and take their values from a finished run
//   Seed    what a stored result is to the fill (the rows forms): the caller's seed arguments; pack() checks them and packs them into host
//           memory the call owns, BEFORE begin (the caller may hand back arrays an earlier call lent out, which begin rewrites);
//           install() puts the packed seed in place of the initial state on the device, after begin (N > 1 only)
//   begin   the earlier loan ends, the pinned result and the device state are sized, the state initialised (k_cc_init / k_nn_init),
//           the slab size decided (before the call allocates anything of its own, as the automatic size reads the free HBM)
//   slab    what is done with one filled slab (compact and append / union / select / accumulate); the state stays on the device.  dom says which pairs
//           its values are: the shard of a triangular slab, or the
//           PcRowsSlab of one slab of a rows slab fill (pc_rows_slab_fill, pc_fill_slabs.hip: f64[m][N] of a range of query rows); begin
//           and end are the triangular walk's
//   end     labels / finish and the D2H copy; the result pointers and counts into the run
//   ship_bytes, ship, merge   several devices: the state a non-root device sends to its slice of the root's staging buffer (0 bytes:
//           nothing travels between devices), and how the root takes the others' state in before its end
// For N <= 1 begin and the walk do nothing on the device.  PcSlabRun is the call as its entry point was given it (pc_slab_check
// refuses in the public calls' order, folds the metric, normalises the flags and settles kk), its working state, and its results.
enum PcSlabKind { PC_SLAB_EDGES, PC_SLAB_COMPONENTS, PC_SLAB_NEAREST, PC_SLAB_TREE, PC_SLAB_BETWEEN, PC_SLAB_AFFINITY, PC_SLAB_HIST };
struct PcSlabRun {
    PcSlabKind kind = PC_SLAB_EDGES;
    const char* who = "";                   // the entry point, for the message texts
    bool outputs = false;                   // every output pointer was there
    int metric = 0, as_distance = 0, strict = 0, k = 0;
    double threshold = 0.0;                 // (nearest: none, stays 0)
    bool by_bars = false;                   // edges: pc_fill_edges_bars -- the predicate is pass(v, bars[s]) || pass(v, bars[t]), the threshold is not read
    const double* bars = nullptr;           // ... the caller's bar[N], host memory
    const int32_t* group = nullptr;         // between, affinity: the caller's labels, host memory, [N]; hist: the same, or NULL (no partition)
    int n_groups = 0;                       // ... and their range
    bool bt_invert = false;                 // ... a similarity table was asked for: the slabs are filled as distances, the fold / finish inverts
    bool want_table = false;                // affinity: the whole [N][n_groups] table is delivered beside the O(N) arrays
    bool allow_unlabelled = false;          // between and affinity, rows forms: a label may be -1, a member of no group
    bool want_gain = false;                 // affinity, rows form: what the queries add to the old genomes' own entries is delivered, [N]
    const int32_t* query = nullptr;         // affinity, rows form: the caller's rows[n_query], host memory (begin counts the queries of each group)
    int64_t slab_bytes = 0;
    bool timed = false;                     // the caller asked for stats: events around the passes over a slab
    int kk = 0;                             // nearest: min(k, N - 1), at least 0 (pc_slab_check)
    int64_t max_pairs = 0;                  // pairs one slab may hold
    pc_stats sum{};                         // the walks' fills, summed
    int32_t n_slabs = 0;                    // ranges the walks cut
    bool pending = false;                   // components / nearest: a slab's passes were launched and, timed, their time not yet added
    // results: the context's pinned memory, set by end
    const int32_t *src = nullptr, *tgt = nullptr, *labels = nullptr, *nbr = nullptr;
    const double* val = nullptr;            // edges: the values; nearest: val[N][kk]
    int64_t n_edges = 0;                    // edges: in the pinned arrays so far; components: pairs that passed (before end: on the other devices)
    int32_t n_components = 0;
    const int64_t *bt_sum = nullptr, *bt_cnt = nullptr;     // between: the four [n_groups][n_groups] arrays
    const int32_t *bt_lo = nullptr, *bt_hi = nullptr;
    const int64_t *af_own_sum = nullptr, *af_near_sum = nullptr, *af_tab_sum = nullptr;      // affinity: [N] / [N] / [N][n_groups] or NULL
    const int32_t *af_own_lo = nullptr, *af_own_hi = nullptr, *af_near_group = nullptr, *af_near_lo = nullptr, *af_near_hi = nullptr;
    const int32_t *af_tab_lo = nullptr, *af_tab_hi = nullptr;
    const int64_t* af_gain_sum = nullptr;   // affinity, rows form with want_gain: [N], else NULL
    const int32_t *af_gain_lo = nullptr, *af_gain_hi = nullptr;
    const int64_t* hist = nullptr;          // hist: [hist_classes][PC_HIST_BINS]
    int32_t hist_classes = 0;               // ... 1 without a partition, 2 with one (class 0 within, class 1 between)
    int64_t hist_pairs = 0;                 // ... the sum of all bins
    int32_t tree_launched = 0;              // tree: rounds enqueued so far (the live ones are counted on the device)
    bool rows_form = false;                 // a rows slab fill (pc_fill_rows_*): edges come row-major, end() sorts them by (target, source)
    int32_t n_query = 0;                    // ... its query rows (all slabs)
};
// The output shapes and the seeds are hidden, and pc_slab_call is static: however their members are inlined, the library's list of
// dynamic symbols stays what it was before they had names.
#pragma GCC visibility push(hidden)
// The output shapes.  An edge list's count is as wide as its entry point declares it: int64_t (edges), int32_t (tree).
template <class Count> struct PcEdgeOut {
    const int32_t **src, **tgt; const double** val; Count* n_edges; int32_t* n_slabs;
    bool all() const { return src && tgt && val && n_edges && n_slabs; }
    void clear() const { if (src) *src = nullptr; if (tgt) *tgt = nullptr; if (val) *val = nullptr; if (n_edges) *n_edges = 0; if (n_slabs) *n_slabs = 0; }
    void take(const PcSlabRun& run) const { *src = run.src; *tgt = run.tgt; *val = run.val; *n_edges = (Count)run.n_edges; *n_slabs = run.n_slabs; }
};
struct PcLabelOut {
    const int32_t** labels; int32_t* n_components; int64_t* n_edges; int32_t* n_slabs;
    bool all() const { return labels && n_components && n_edges && n_slabs; }
    void clear() const { if (labels) *labels = nullptr; if (n_components) *n_components = 0; if (n_edges) *n_edges = 0; if (n_slabs) *n_slabs = 0; }
    void take(const PcSlabRun& run) const { *labels = run.labels; *n_components = run.n_components; *n_edges = run.n_edges; *n_slabs = run.n_slabs; }
};
struct PcListOut {
    const int32_t** nbr; const double** val; int32_t* k; int32_t* n_slabs;
    bool all() const { return nbr && val && k && n_slabs; }
    void clear() const { if (nbr) *nbr = nullptr; if (val) *val = nullptr; if (k) *k = 0; if (n_slabs) *n_slabs = 0; }
    void take(const PcSlabRun& run) const { *nbr = run.nbr; *val = run.val; *k = run.kk; *n_slabs = run.n_slabs; }
};
struct PcTableOut {
    const int64_t **sum, **count; const int32_t **lo, **hi; int32_t* n_slabs;
    bool all() const { return sum && count && lo && hi && n_slabs; }
    void clear() const { if (sum) *sum = nullptr; if (count) *count = nullptr; if (lo) *lo = nullptr; if (hi) *hi = nullptr; if (n_slabs) *n_slabs = 0; }
    void take(const PcSlabRun& run) const { *sum = run.bt_sum; *count = run.bt_cnt; *lo = run.bt_lo; *hi = run.bt_hi; *n_slabs = run.n_slabs; }
};
struct PcGenomeTableOut {
    const int64_t** own_sum; const int32_t **own_lo, **own_hi, **near_group; const int64_t** near_sum; const int32_t **near_lo, **near_hi;
    const int64_t** tab_sum; const int32_t **tab_lo, **tab_hi; int32_t* n_slabs;
    bool all() const { return own_sum && own_lo && own_hi && near_group && near_sum && near_lo && near_hi && tab_sum && tab_lo && tab_hi && n_slabs; }
    void clear() const {
        if (own_sum) *own_sum = nullptr; if (own_lo) *own_lo = nullptr; if (own_hi) *own_hi = nullptr; if (near_group) *near_group = nullptr;
        if (near_sum) *near_sum = nullptr; if (near_lo) *near_lo = nullptr; if (near_hi) *near_hi = nullptr;
        if (tab_sum) *tab_sum = nullptr; if (tab_lo) *tab_lo = nullptr; if (tab_hi) *tab_hi = nullptr; if (n_slabs) *n_slabs = 0;
    }
    void take(const PcSlabRun& run) const {
        *own_sum = run.af_own_sum; *own_lo = run.af_own_lo; *own_hi = run.af_own_hi; *near_group = run.af_near_group;
        *near_sum = run.af_near_sum; *near_lo = run.af_near_lo; *near_hi = run.af_near_hi;
        *tab_sum = run.af_tab_sum; *tab_lo = run.af_tab_lo; *tab_hi = run.af_tab_hi; *n_slabs = run.n_slabs;
    }
};
struct PcHistOut {
    const int64_t** hist; int32_t* n_classes; int64_t* n_pairs; int32_t* n_slabs;
    bool all() const { return hist && n_classes && n_pairs && n_slabs; }
    void clear() const { if (hist) *hist = nullptr; if (n_classes) *n_classes = 0; if (n_pairs) *n_pairs = 0; if (n_slabs) *n_slabs = 0; }
    void take(const PcSlabRun& run) const { *hist = run.hist; *n_classes = run.hist_classes; *n_pairs = run.hist_pairs; *n_slabs = run.n_slabs; }
};
struct PcPlacementOut {                     // the rows form of the affinity fill: the per-query arrays, and the gain of the old genomes
    PcGenomeTableOut rows; const int64_t** gain_sum; const int32_t **gain_lo, **gain_hi;
    bool all() const { return rows.all() && gain_sum && gain_lo && gain_hi; }
    void clear() const { rows.clear(); if (gain_sum) *gain_sum = nullptr; if (gain_lo) *gain_lo = nullptr; if (gain_hi) *gain_hi = nullptr; }
    void take(const PcSlabRun& run) const { rows.take(run); *gain_sum = run.af_gain_sum; *gain_lo = run.af_gain_lo; *gain_hi = run.af_gain_hi; }
};
// The seeds: the caller's arguments first (an entry point brace-initialises them), then what pack() made of them.
struct PcNoSeed {                           // edges: a stored list needs nothing on the device, the caller merges the two lists
    int pack(const pc_ctx*, const PcSlabRun&, const int32_t*, int) { return PC_OK; }
    int install(pc_ctx*, PcSlabRun&) const { return PC_OK; }
};
struct PcLabelSeed {                        // components: the stored labelling, int32[N] or NULL, as the initial parent[]
    const int32_t* labels; std::vector<int32_t> packed;
    int pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows);
    int install(pc_ctx* c, PcSlabRun& run) const;
};
struct PcTreeSeed {                         // tree: the stored tree's n edges, as keys, the resident forest
    const int32_t *src, *tgt; const double* val; int32_t n; std::vector<unsigned long long> keys;
    int pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows);
    int install(pc_ctx* c, PcSlabRun& run) const;
};
struct PcNearestSeed {                      // nearest: the stored lists [N][k_seed], as key[N][kk] / idx[N][kk] (none: ks == 0), the resident lists
    const int32_t* nbr; const double* val; int32_t k_seed; int ks = 0; std::vector<unsigned long long> keys; std::vector<int32_t> idx;
    int pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows);
    int install(pc_ctx* c, PcSlabRun& run) const;
};
struct PcBetweenSeed {                      // between: the stored table, four [G][G] arrays in the result layout and the call's direction (all NULL:
    const int64_t *sum, *count; const int32_t *lo, *hi;     // none), as the raw accumulator's image (pc_between_bytes; empty: no seed)
    std::vector<unsigned long long> image;
    int pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows);
    int install(pc_ctx* c, PcSlabRun& run) const;
};
struct PcHistSeed {                         // hist: the stored histogram, i64[classes][PC_HIST_BINS] in the call's direction (NULL: none), as the
    const int64_t* hist;                    // raw state's bins (distances; empty: no seed)
    std::vector<unsigned long long> image;
    int pack(const pc_ctx* c, const PcSlabRun& run, const int32_t* rows, int n_rows);
    int install(pc_ctx* c, PcSlabRun& run) const;
};
#pragma GCC visibility pop
#define PC_SLAB_FILL(Name, Dom, tag, text, KIND, OUT, SEED)                                                                             \
    struct Name {                                                                                                                       \
        static constexpr const char *what = text, *who = "pc_fill_" tag, *range = "pc:fill_" tag, *multi_range = "pc:multi_fill_" tag; \
        static constexpr PcSlabKind kind = KIND;                                                                                        \
        using Out = OUT; using Seed = SEED;                                                                                             \
        static int begin(pc_ctx* c, PcSlabRun& run);                                                                                    \
        static int slab(pc_ctx* c, PcSlabRun& run, const double* slab, int64_t Lp, const Dom& dom);                                     \
        static int end(pc_ctx* c, PcSlabRun& run);                                                                                      \
        static size_t ship_bytes(const pc_ctx* root, const PcSlabRun& run);                                                             \
        static int ship(pc_ctx* c, pc_ctx* root, PcSlabRun& run, void* stage, int slot, int n_foreign);                                 \
        static int merge(const std::vector<pc_ctx*>& ctx, std::vector<PcSlabRun>& runs, const void* stage, int n_foreign, float* ms_exchange); \
    }
PC_SLAB_FILL(PcEdgesFill, PcSlabDomain, "edges", "an edge-list fill", PC_SLAB_EDGES, PcEdgeOut<int64_t>, PcNoSeed);
PC_SLAB_FILL(PcComponentsFill, PcSlabDomain, "components", "a components fill", PC_SLAB_COMPONENTS, PcLabelOut, PcLabelSeed);
PC_SLAB_FILL(PcNearestFill, PcSlabDomain, "nearest", "a nearest-neighbours fill", PC_SLAB_NEAREST, PcListOut, PcNearestSeed);
PC_SLAB_FILL(PcTreeFill, PcSlabDomain, "tree", "a tree fill", PC_SLAB_TREE, PcEdgeOut<int32_t>, PcTreeSeed);
PC_SLAB_FILL(PcBetweenFill, PcSlabDomain, "between", "a between-groups fill", PC_SLAB_BETWEEN, PcTableOut, PcBetweenSeed);
PC_SLAB_FILL(PcAffinityFill, PcSlabDomain, "affinity", "an affinity fill", PC_SLAB_AFFINITY, PcGenomeTableOut, PcNoSeed);
PC_SLAB_FILL(PcHistFill, PcSlabDomain, "hist", "a distribution fill", PC_SLAB_HIST, PcHistOut, PcHistSeed);
#undef PC_SLAB_FILL
// What every entry point of these fills does around its driver: the outputs cleared before anything else, kind / outputs / timed into
// the run (whose call fields the entry point has set), drive(), and on PC_OK the results into the outputs and the run's own stats
// into stats[0] (several devices: the root's; multi_slab_fill writes the others').
template <class Fill, class Out = typename Fill::Out, class Drive> static int pc_slab_call(PcSlabRun& run, const Out& out, pc_stats* stats, Drive drive) {
    out.clear();
    run.kind = Fill::kind; run.outputs = out.all(); run.timed = stats != nullptr;
    const int rc = drive();
    if (rc != PC_OK) return rc;
    out.take(run);
    if (stats) stats[0] = run.sum;
    return PC_OK;
}
int pc_slab_check(const pc_ctx* c, PcSlabRun& run, const char* what);
template <class Fill> int pc_slab_fill(pc_ctx* c, PcSlabRun& run);
template <class Fill> int pc_slab_stretch(pc_ctx* c, PcSlabRun& run, int ta, int tb);
// `bytes` of device c's state into the root's staging buffer, on c's stream
static int pc_ship(pc_ctx* c, pc_ctx* root, void* dst, const void* src, size_t bytes) {
    if (c->device == root->device) PC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    else PC_HIP(hipMemcpyPeerAsync(dst, root->device, src, c->device, bytes, c->stream));
    return PC_OK;
}

// DP cells per target genome into c->target_cost, once per upload: one COUNT walk over all pairs (pc_upload.hip).  The context must
// be unsharded (rank 0 of 1 in force) and idle; no deal is installed or left behind.
int pc_count_target_costs(pc_ctx* c);

// What a fill delivers: one metric into one array, or -- mask != 0, a JOINT fill (pc_fill_joint*, pc_fill_pairs_joint*) -- metric m of
// every set bit m of mask into joint[m], all off one plan and one alignment pass.  A joint fill plans, aligns and is accounted as the
// peq fill it walks as, so its `metric` is PC_PEQ wherever a stage asks for one.
struct PcFillOut {
    int metric; double* out;
    uint32_t mask; double* joint[6];
    PcFillOut(int metric_, double* out_) : metric(metric_), out(out_), mask(0), joint{} {}
    PcFillOut(uint32_t mask_, void* const joint_[6]) : metric(PC_PEQ), out(nullptr), mask(mask_), joint{} {
        for (int m = 0; m < 6; ++m) joint[m] = (mask >> m & 1u) ? (double*)joint_[m] : nullptr;
    }
};
#define PC_JOINT_ALL 0x3fu                  // bits PC_GCS ... PC_PEQ

// the whole fill of the shard in force into out (pc_fill.hip): what pc_fill_dev / pc_fill_shard_dev run, and every slab of a slab walk
int fill_impl(pc_ctx* c, int metric, int as_distance, double* out, int condensed, hipStream_t st, pc_stats* stats);
// aai / peq / a joint set: COUNT, then plan -> align -> reduce, in one piece or in chunks (pc_align.hip)
int fill_aligned(pc_ctx* c, const PcFillOut& o, int ppos, int as_distance, int condensed, hipStream_t st, pc_stats& local, bool timed);
// a rows fill (dom.rows; out: f64[rows->nrows][N]), a groups fill (dom.groups; out: f64[L]) or a pair-list fill (dom.pairs; out: f64[L]
// in the caller's order) once its domain tables are on the device: the set metrics in one launch of the domain's walker, aai / peq
// chunked over ranges of query rows / of row blocks / of blocks of slots (pc_align.hip).  A joint set: a pair-list fill only
int fill_units(pc_ctx* c, const PcUnitDomain& dom, const PcFillOut& o, int ppos, int as_distance, hipStream_t st, pc_stats& local, bool timed);
