// pc_align.hip -- the alignment fill of aai / peq in libphamclust_hip.so: the class launches, the plan budget and chunking,
// the alignment-sliced multi-GPU route (pc_plan_dev, pc_align_slice_dev, pc_reduce_dev) and pc_align_pairs.
//
// Fill plan for aai/peq (all on one stream, one small read-back in the middle):
//   1 COUNT walk     per pair: alignments; per column gene: bucket sizes; totals
//   2 scans          pair -> first result slot; gene -> bucket start; gene -> first task
//   3 read-back      alignment total + task range per kernel variant (a few words)
//   4 ENUM walk      (row gene, result slot) scattered into the column gene's bucket
//   5 K4 launches    one per kernel variant present, wave tasks of <= 64 row sequences
//   6 REDUCE walk    best match per anchor gene, fp64 weighted mean, af, round -> out (a joint fill: -> one array per metric asked for)
// Bucketing by column gene is what lets a wave build one substitution profile and stream
// many row sequences through it; results are written pair-major so step 6 reads them
// contiguously and in the canonical order (pham id, anchor gene, other gene).
#include <numeric>

#include "pc_host.h"

// Step 5 of the plan: launch the alignment kernels for every launch class that has tasks.  Classes are
// independent (disjoint result slots), so their launches are spread over the caller's stream and
// seven auxiliary streams: the drain of one class overlaps the next one's start.
static int small_launch_min() {              // fewest tasks that earn a one- / two-wave mode a launch of its own
    static const int v = [] { const char* e = getenv("PC_SMALL_LAUNCH_MIN"); const int x = e ? atoi(e) : 0; return x > 0 ? x : 192; }();
    return v;
}
static int run_align_classes(pc_ctx* c, const PcTask* task_list, const uint32_t* task_begin /*[nlc+1]*/, const int32_t* cls_max_lb,
                             uint2* res, hipStream_t st, pc_stats* stats, int ppos) {
    const int nbase = c->ncls_all;
    // One launch = a run of neighbouring launch classes of ONE base class, run in the workgroup shape of the first of them.  The
    // modes of a base class follow each other in the sorted task list (own shape, two waves, one wave), so a small-task mode with
    // too few tasks to pay for a launch of its own -- every launch holds its hardware queue until its last workgroup is done --
    // rides at the end of the launch before it: correct in any shape, merely less snug.
    struct Launch { uint32_t begin, end; int base, mode, max_lb; };
    std::vector<Launch> launches;
    for (int b = 0; b < nbase; ++b) {
        const uint32_t* tb = task_begin + (size_t)b * PC_WAVE_MODES;
        if (tb[PC_WAVE_MODES] == tb[0]) continue;
        const uint32_t n0 = tb[1] - tb[0], n1 = tb[2] - tb[1], n2 = tb[3] - tb[2];
        // (the wide variants' tasks are hundreds of times a small gene's, and their one- / two-row tasks run on another kernel
        // altogether -- narrow strip-mined passes: always worth a launch)
        const int bv = pc_class_variant(b);
        const uint32_t least = (bv >= 0 && pc_nw_variant_w(bv) >= 32) ? 1u : (uint32_t)small_launch_min();
        const bool own2 = n2 >= least, own1 = n1 + (own2 ? 0u : n2) >= least;      // one-wave tasks alone? two-wave (+ folded one-wave) alone?
        uint32_t at = tb[0];
        const int max_lb = cls_max_lb[b * PC_WAVE_MODES];
        auto put = [&](uint32_t n, int mode) { if (n) launches.push_back({at, at + n, b, mode, max_lb}); at += n; };
        if (own1) { put(n0, PC_MODE_CLASS); put(n1 + (own2 ? 0u : n2), n1 ? PC_MODE_TWO_WAVES : PC_MODE_ONE_WAVE); }
        else put(n0 + n1 + (own2 ? 0u : n2), n0 ? PC_MODE_CLASS : n1 ? PC_MODE_TWO_WAVES : PC_MODE_ONE_WAVE);
        if (own2) put(n2, PC_MODE_ONE_WAVE);
    }
    if (launches.empty()) return PC_OK;
    // longest tasks first (a task's duration grows with its column gene's length): the tail of the fill is then made
    // of short tasks
    std::stable_sort(launches.begin(), launches.end(), [&](const Launch& x, const Launch& y) {
        if (x.max_lb != y.max_lb) return x.max_lb > y.max_lb;
        return x.base != y.base ? x.base < y.base : x.mode < y.mode;
    });
    // Scratch slab (sized before anything is launched, never re-allocated between launches).  The general kernel's launches share
    // its first region and stay in order on the caller's stream.  Every strip-mined launch gets a region of its OWN behind it and one
    // of the context's long-task streams (pc_ctx::lng): a collection's long-gene launches are few tasks of tens of milliseconds each -- a 6,600 x 6,600
    // alignment on one wave takes 47 ms -- and lined up on one stream they were the critical path of the fill (synth_real(5000):
    // three strip launches, 112 + 41 + 48 ms end to end, the last two on a nearly empty chip, under a fill of 243 ms).  Only
    // what does not fit PC_SLAB_BUDGET (3 GB) shares the first region, in order, as before.
    // percent-positives: systolic where the profile cell can run (it reads "positive" from a table), general kernel elsewhere
    auto launch_variant = [&](const Launch& l) { const int v = pc_class_variant(l.base); return (ppos && !pc_nw_ppos_systolic(v, l.max_lb)) ? pc_nw_ppos_variant(l.max_lb) : v; };
    auto uses_slab = [&](const Launch& l) { const int v = launch_variant(l); return v < 0 || pc_nw_launch_is_strip(v, l.max_lb, l.mode, ppos); };
    struct Region { size_t off, bytes; bool own; };
    std::vector<Region> region(launches.size(), Region{0, 0, false});
    static const size_t slab_budget = [] { const char* e = getenv("PC_SLAB_BUDGET"); const long long v = e ? atoll(e) : 0; return v > 0 ? (size_t)v : (size_t)3 << 30; }();
    static const bool strips_in_line = getenv("PC_STRIP_STREAMS") && !strcmp(getenv("PC_STRIP_STREAMS"), "0");     // A/B: the r04 order
    size_t sbytes = 0;
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    auto lay_out = [&](bool in_line) {                                    // regions of the slab; in_line: every strip-mined launch shares the first
        size_t shared = 0, own_total = 0;
        std::fill(region.begin(), region.end(), Region{0, 0, false});
        for (const Launch& l : launches) if (launch_variant(l) < 0) shared = std::max(shared, pc_nw_fallback_scratch_bytes(l.max_lb));
        for (size_t i = 0; i < launches.size(); ++i) {
            const Launch& l = launches[i];
            const int v = launch_variant(l);
            if (v < 0 || !pc_nw_launch_is_strip(v, l.max_lb, l.mode, ppos)) continue;
            const size_t need = up256(pc_nw_strip_launch_bytes(l.mode, (int)(l.end - l.begin), c->max_gene_len, c->n_cu, ppos));
            if (!in_line && c->n_streams > 1 && own_total + need <= slab_budget) { region[i] = Region{own_total, need, true}; own_total += need; }
            else shared = std::max(shared, pc_nw_strip_scratch_bytes(c->max_gene_len, c->n_cu));
        }
        shared = up256(shared);
        for (size_t i = 0; i < launches.size(); ++i) {
            if (region[i].own) region[i].off += shared;
            else if (uses_slab(launches[i])) region[i] = Region{0, shared, false};
        }
        sbytes = shared + own_total;
        return own_total;
    };
    const size_t own_total = lay_out(strips_in_line);
    if (sbytes) {
        int rc = c->b_scratch.ensure(sbytes);
        // The slab's own regions can reach 3 GB + 1 GB shared, and their size follows the chip and the longest gene, not the chunk: a
        // chunked fill on a nearly full device would halve its chunk again and again without the slab getting any smaller.  So: once
        // more with every strip-mined launch in line on the shared region (fewer bytes, same values) before the chunk is given up.
        if (rc == PC_ERR_NOMEM_INTERNAL && own_total > 0) { lay_out(true); rc = sbytes ? c->b_scratch.ensure(sbytes) : PC_OK; }
        if (rc != PC_OK) return rc;
    }
    // Launch classes of one register tier, cell and workgroup size share ONE launch (k_nw_systolic_tier, pc_nw_fuse_key): the
    // hardware queues run launches back to back, each waiting for the last workgroup of the one before it, and a fill's ~80
    // launches cost it a task's duration each -- bundled they are ~15, each holding more tasks than the chip does at once.
    // Groups keep the order of their first member (longest column genes first); inside a group the classes follow that order too.
    struct Group { int key; std::vector<int> members; };
    std::vector<Group> groups;
    for (int i = 0; i < (int)launches.size(); ++i) {
        const Launch& l = launches[i];
        const int key = pc_nw_fuse_key(launch_variant(l), l.max_lb, ppos, pc_class_compare_only(l.base), l.mode);
        size_t g = groups.size();
        if (key >= 0) for (size_t k = 0; k < groups.size(); ++k) if (groups[k].key == key && groups[k].members.size() < PC_FUSE_MAX_SEGMENTS) { g = k; break; }
        if (g == groups.size()) groups.push_back({key, {}});
        groups[g].members.push_back(i);
    }
    // Launches of little work (fewer wave-tasks than four rounds of the chip's wave slots: a fill has two dozen, a millisecond or less
    // each) are ISSUED first: at the head of the streams they are done within the fill's first milliseconds.  In the order above the
    // last of them sat behind the launch that runs for most of the fill, in its hardware queue, and ran one after the other on an
    // empty chip when it ended -- the fill's fixed cost (profiles/r05/experiments/k4_fill_timeline.txt: 3.2 ms at N = 5,000, 2.6 of a
    // 75-ms rank of the 8-rank shard).  Worth -0.5 % at N = 2,000, nothing at 5,000, -1.0 % for that rank: T(w) = 3.3 + 548 / w.
    {
        const uint64_t small_below = (uint64_t)4 * 32 * (uint64_t)(c->n_cu > 0 ? c->n_cu : 256);
        std::stable_partition(groups.begin(), groups.end(), [&](const Group& grp) {
            uint64_t wave_tasks = 0;
            for (int i : grp.members) {
                const Launch& l = launches[i];
                if (region[i].bytes) return false;                             // (launches on the scratch slab keep their place)
                wave_tasks += (uint64_t)(l.end - l.begin) * (l.mode == PC_MODE_ONE_WAVE ? 1u : l.mode == PC_MODE_TWO_WAVES ? 2u : 4u);
            }
            return wave_tasks < small_below;
        });
    }
    constexpr int kAux = pc_ctx::kAux;
    const int n_aux = std::min((int)groups.size(), c->n_streams) - 1;        // auxiliary streams this fill uses
    int n_long = 0;                                                          // launches with a scratch region of their own: on the long-task streams
    for (const Region& rg : region) if (rg.own) ++n_long;
    n_long = std::min(n_long, (int)pc_ctx::kLong);
    PC_HIP(hipEventRecord(c->aux_ev[kAux], st));
    for (int k = 0; k < n_aux; ++k) PC_HIP(hipStreamWaitEvent(c->aux[k], c->aux_ev[kAux], 0));
    for (int k = 0; k < n_long; ++k) PC_HIP(hipStreamWaitEvent(c->lng[k], c->aux_ev[kAux], 0));
    int slot = 0, long_slot = 0, first_error = PC_OK;
    for (const Group& grp : groups) {
        int rc = PC_OK;
        if (grp.key >= 0) {
            PcNwSegment segs[PC_FUSE_MAX_SEGMENTS];
            int ns = 0;
            for (int i : grp.members) {
                const Launch& l = launches[i];
                segs[ns++] = {l.begin, l.end - l.begin, launch_variant(l), l.max_lb, pc_class_compare_only(l.base), l.mode};
            }
            hipStream_t ls = slot == 0 ? st : c->aux[slot - 1];
            rc = pc_launch_nw_group(segs, ns, c->dev, task_list, c->b_bucket_row.as<int32_t>(), nullptr /* result slot = position in the sorted list */,
                                    res, ppos, c->tie_rule, ls);
        } else {
            const Launch& l = launches[grp.members[0]];
            const int nt = (int)(l.end - l.begin);
            const int variant = launch_variant(l);
            // launches that share the slab's first region stay in order on the caller's stream
            const Region& rg = region[grp.members[0]];
            const bool slab = rg.bytes != 0;
            hipStream_t ls = rg.own ? c->lng[long_slot++ % n_long] : ((slab || slot == 0) ? st : c->aux[slot - 1]);
            rc = pc_launch_nw(variant, c->dev, task_list + l.begin, nt, c->b_bucket_row.as<int32_t>(),
                              nullptr, res, slab ? (void*)((char*)c->b_scratch.p + rg.off) : nullptr,
                              slab ? rg.bytes : 0, l.max_lb, ppos, c->tie_rule, pc_class_compare_only(l.base), ls, l.mode, c->max_gene_len);
        }
        if (rc != PC_OK) { first_error = rc; break; }
        if (stats) ++stats->n_align_launches;
        if (!(grp.key < 0 && region[grp.members[0]].own)) slot = (slot + 1) % (n_aux + 1);
    }
    // join the auxiliary streams back into the caller's stream -- also after a failed launch, so that what was
    // already queued on them is ordered before anything the caller does next
    for (int k = 0; k < n_aux; ++k) {
        PC_HIP(hipEventRecord(c->aux_ev[k], c->aux[k]));
        PC_HIP(hipStreamWaitEvent(st, c->aux_ev[k], 0));
    }
    for (int k = 0; k < n_long; ++k) {
        PC_HIP(hipEventRecord(c->lng_ev[k], c->lng[k]));
        PC_HIP(hipStreamWaitEvent(st, c->lng_ev[k], 0));
    }
    return first_error;
}

// ---- the three stages of an aai / peq fill.  pc_fill* run them back to back; the alignment-sliced multi-GPU route
// (pc_plan_dev, pc_align_slice_dev, pc_reduce_dev) runs them with a collective between the last two.

// Memory-bounded batching (the reference never holds more than ~10,000 pairs per CPU in flight, matrix.py:474-493, and so
// runs any N).  The plan buffers of an aai / peq fill take PC_PLAN_BYTES_PER_ALIGNMENT bytes per alignment; when that
// exceeds the budget -- or the 2^31-1 alignments a plan can index -- the fill runs plan -> align -> reduce over successive
// ranges of the shard's target genomes.  Cutting by target keeps every pair's alignments in one chunk.
#define PC_PLAN_BYTES_PER_ALIGNMENT 56
#define PC_PLAN_MAX_ALIGNMENTS 0x7ffffffeLL

// Pure host arithmetic, exported for tests: cut [0, n) into consecutive ranges whose sums stay <= max_per_chunk (a single
// element above it gets a range of its own).  chunk_begin receives the range starts followed by n (at most cap entries are
// written); returns the number of ranges.
extern "C" int pc_chunk_plan(const uint64_t* count, int n, uint64_t max_per_chunk, int32_t* chunk_begin, int cap) {
    if (!count || n < 0 || max_per_chunk == 0) { pc_set_error("pc_chunk_plan: bad argument"); return PC_ERR_ARG; }
    int nch = 0, start = 0; uint64_t run = 0;
    auto put = [&](int v) { if (chunk_begin && nch < cap) chunk_begin[nch] = v; ++nch; };
    if (n > 0) put(0);
    for (int k = 0; k < n; ++k) {                      // (the same rule as fill_aligned's loop: extend while the sum stays within the limit)
        if (k > start && (run + count[k] > max_per_chunk || run + count[k] < run)) { put(k); run = 0; start = k; }
        run += count[k];
    }
    if (chunk_begin && nch < cap) chunk_begin[nch] = n;
    return nch;
}

// The tree fill's key (the C-ABI header states it), host arithmetic as the rule above: packed and unpacked for callers and tests.
extern "C" uint64_t pc_tree_key(int32_t micro, int32_t s, int32_t t) {
    if (micro < 0 || micro > PC_TREE_MICRO_MAX || s < 0 || t <= s || t >= PC_TREE_MAX_GENOMES) return (uint64_t)PC_TREE_NONE;
    return (uint64_t)pc_tree_key_of(micro, s, t);
}
extern "C" int pc_tree_key_parts(uint64_t key, int32_t* micro, int32_t* s, int32_t* t) {
    const int m = pc_tree_key_micro(key), ks = pc_tree_key_s(key), kt = pc_tree_key_t(key);
    const bool ok = m <= PC_TREE_MICRO_MAX && ks < kt;
    if (micro) *micro = ok ? m : -1;
    if (s) *s = ok ? ks : -1;
    if (t) *t = ok ? kt : -1;
    if (!ok) { pc_set_error("pc_tree_key_parts: %llx is no key", (unsigned long long)key); return PC_ERR_ARG; }
    return PC_OK;
}

extern "C" int pc_set_plan_budget(pc_ctx* c, int64_t bytes) {
    if (!c || bytes < 0) { pc_set_error("pc_set_plan_budget: bad argument"); return PC_ERR_ARG; }
    c->plan_budget = bytes;
    return PC_OK;
}

// bytes one chunk's plan buffers may take: the caller's figure (pc_set_plan_budget / PC_PLAN_BYTES), else half of what
// is free now plus what the grow-only plan buffers already hold
static int64_t plan_budget_bytes(pc_ctx* c) {
    if (c->plan_budget > 0) return c->plan_budget;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return (int64_t)16 << 30; }
    const size_t held = c->b_key0.cap + c->b_key1.cap + c->b_val0.cap + c->b_val1.cap + c->b_flags.cap + c->b_excl.cap + c->b_alias.cap +
                        c->b_bucket_row.cap + c->b_res.cap + c->b_sort_tmp.cap;
    return (int64_t)((free_b + held) / 2);
}
static void release_plan_buffers(pc_ctx* c) {
    DevBuf* bufs[] = {&c->b_key0, &c->b_key1, &c->b_val0, &c->b_val1, &c->b_flags, &c->b_excl, &c->b_alias, &c->b_bucket_row, &c->b_res, &c->b_sort_tmp,
                      &c->b_tasks, &c->b_tasks_sorted};
    for (DevBuf* b : bufs) b->release();
}

// COUNT over the whole shard: alignments per pair (the reference's loop nest, metrics.py:204-224) into b_na, and the
// totals (alignments, cells, residue bytes); one read-back.
static int stage_count(pc_ctx* c, int condensed, hipStream_t st, uint64_t tot[3]) {
    PcRange range("pc:count");
    int rc = PC_OK;
    const PcDev& d = c->dev;
    const int64_t Lp = c->shard_pairs;
    if (d.G > 0 && c->min_gene_len == 0) {
        pc_set_error("fill: an empty translation cannot be aligned (aai/peq); the reference fails on it too"); return PC_ERR_DATA;
    }
    if ((rc = c->b_na.ensure((Lp + 1) * 4)) || (rc = c->b_off.ensure((Lp + 1) * 4)) || (rc = c->b_totals.ensure(64))) return rc;
    PC_HIP(hipMemsetAsync(c->b_na.p, 0, (Lp + 1) * 4, st));
    PC_HIP(hipMemsetAsync(c->b_totals.p, 0, 64, st));
    PcWalkArgs a; memset(&a, 0, sizeof(a));
    a.na = c->b_na.as<uint32_t>(); a.totals = c->b_totals.as<unsigned long long>();
    a.as_distance = 0; a.condensed = condensed;
    if ((rc = pc_launch_walk(PCW_COUNT, d, c->shard, a, st))) return rc;
    uint64_t* h_tot = (uint64_t*)(c->h_plan.as<uint32_t>() + 1000);
    PC_HIP(hipMemcpyAsync(h_tot, c->b_totals.p, 24, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));                                     // first read-back: the batch size
    tot[0] = h_tot[0]; tot[1] = h_tot[1]; tot[2] = h_tot[2];
    return PC_OK;
}

// alignments behind each owned target genome (a second COUNT walk, only when a fill has to be cut into chunks)
static int count_per_target(pc_ctx* c, int condensed, hipStream_t st, std::vector<uint64_t>& per_owned) {
    int rc = PC_OK;
    const int N = c->dev.N;
    if ((rc = c->b_aln_t.ensure((size_t)N * 8))) return rc;
    PC_HIP(hipMemsetAsync(c->b_aln_t.p, 0, (size_t)N * 8, st));
    PcWalkArgs a; memset(&a, 0, sizeof(a));
    a.totals = c->b_totals.as<unsigned long long>() + 5;                  // (slots 5..7: scratch, nobody reads them)
    a.aln_t = c->b_aln_t.as<unsigned long long>(); a.condensed = condensed;
    if ((rc = pc_launch_walk(PCW_COUNT, c->dev, c->shard, a, st))) return rc;
    std::vector<uint64_t> all(N);
    PC_HIP(hipMemcpyAsync(all.data(), c->b_aln_t.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    per_owned.resize(c->h_owned.size());
    for (size_t k = 0; k < c->h_owned.size(); ++k) per_owned[k] = all[c->h_owned[k]];
    return PC_OK;
}

// Which walk a stage launches, over which slots: the owned targets [k0, k1) of the context's shard (k_walk; slot arrays indexed
// by the shard-local pair index), or -- rows != NULL -- the query rows [k0, k1) of a rows fill (k_walk_rows; slot arrays
// [k1 - k0][N], filled for that range alone), or -- groups != NULL -- the row blocks [k0, k1) of a groups fill (k_walk_groups; slot
// arrays hold that range's slots, first slot block_slot[k0]), or -- dom.pairs -- the blocks [k0, k1) of a pair-list fill (k_walk_pairs;
// slot arrays hold that range's slots, first slot k0 * PC_PAIR_BLOCK).
static PcPairs pairs_from(const PcPairsHost& ph, int k0) {
    PcPairs sub = ph.dev;
    sub.slot_base = (int64_t)k0 * PC_PAIR_BLOCK;
    return sub;
}
static PcShard shard_range(const pc_ctx* c, int k0, int k1) {
    PcShard sub = c->shard;
    sub.nown = k1 - k0; sub.owned = c->shard.owned + k0; sub.lbase = c->shard.lbase + k0; sub.ident = c->shard.ident && k0 == 0;
    return sub;
}
static int walk_domain(pc_ctx* c, int mode, const PcUnitDomain& dom, int k0, int k1, const PcWalkArgs& a, hipStream_t st) {
    if (dom.rows) return pc_launch_walk_rows(mode, c->dev, *dom.rows, k0, k1, a, st);
    if (dom.groups) {
        PcGroups sub = dom.groups->dev;
        sub.slot_base = dom.groups->block_slot[k0];
        return pc_launch_walk_groups(mode, c->dev, sub, dom.groups->block_tile[k0], dom.groups->block_tile[k1], a, st);
    }
    if (dom.pairs) return pc_launch_walk_pairs(mode, c->dev, pairs_from(*dom.pairs, k0), k0, k1, a, st);
    return pc_launch_walk(mode, c->dev, shard_range(c, k0, k1), a, st);
}
// ... and the JOINT walk, which exists over the shard's targets and over the blocks of a pair list
static int walk_domain_joint(pc_ctx* c, const PcUnitDomain& dom, int k0, int k1, const PcJointArgs& a, hipStream_t st) {
    if (dom.rows || dom.groups) { pc_set_error("reduce: no joint walk over a rows or groups domain"); return PC_ERR_ARG; }
    if (dom.pairs) return pc_launch_walk_pairs_joint(c->dev, pairs_from(*dom.pairs, k0), k0, k1, a, st);
    return pc_launch_walk_joint(c->dev, shard_range(c, k0, k1), a, st);
}

// PLAN of the owned targets (or the units of dom) [k0, k1) holding A alignments (b_na is filled): scan, ENUM, sort, distinct alignments, tasks
// sorted by launch class.  Leaves its results in the context's work buffers and c->plan; two small read-backs.
static int stage_plan(pc_ctx* c, int ppos, int condensed, hipStream_t st, int k0, int k1, uint64_t A, const PcUnitDomain& dom = PcUnitDomain{}) {
    int rc = PC_OK;
    PcRange range("pc:plan");
    PlanningScope planning;
    const PcDev& d = c->dev;
    pc_ctx::PlanState& P = c->plan;
    P.valid = false; P.ppos = ppos; P.condensed = condensed; P.A = (int64_t)A; P.n_distinct = 0; P.ntasks = 0; P.tb.assign(c->nlc + 1, 0);
    P.k0 = k0; P.k1 = k1; P.whole = !dom.any() && c->world == 1 && condensed == 1 && k0 == 0 && k1 == c->shard.nown;
    memset(&P.st, 0, sizeof(P.st));
    pc_stats& local = P.st;
    const int64_t base = dom.any() ? 0 : c->h_lbase[k0];
    const int64_t Lc = dom.any() ? dom.slots(k0, k1, d.N) : c->h_lbase[k1] - base;
    local.n_pairs = Lc;
    local.n_alignments = (int64_t)A;
    if (A > (uint64_t)PC_PLAN_MAX_ALIGNMENTS) {
        pc_set_error("plan: %llu alignments behind ONE target genome exceed the 2^31-2 a plan can index", (unsigned long long)A); return PC_ERR_LIMIT;
    }
    const int U = d.U;
    const int ncls = c->nlc;
    const int64_t tmp_fixed = std::max<int64_t>(Lc + 1, U + 1);
    if ((rc = c->b_start_q.ensure((U + 1) * 4)) || (rc = c->b_end_q.ensure((U + 1) * 4)) || (rc = c->b_ntask_q.ensure((U + 1) * 4)) ||
        (rc = c->b_task_off_q.ensure((U + 1) * 4)) || (rc = c->b_scan_tmp.ensure(pc_scan_tmp_elems(tmp_fixed) * 4)) || (rc = c->b_plan.ensure(4096)))
        return rc;
    // alignment slot of a pair = exclusive scan of the chunk's counts (slots start at 0 in every chunk)
    if (Lc > 0 && (rc = pc_scan_exclusive_u32(c->b_na.as<uint32_t>() + base, c->b_off.as<uint32_t>() + base, Lc, c->b_scan_tmp.as<uint32_t>(),
                                              (int64_t)(c->b_scan_tmp.cap / 4), st))) return rc;
    PcWalkArgs a; memset(&a, 0, sizeof(a));
    a.as_distance = 0; a.condensed = condensed;
    a.off = c->b_off.as<uint32_t>();
    uint32_t* const h_plan = c->h_plan.as<uint32_t>();
    uint64_t* h_tot = (uint64_t*)(h_plan + 1000);
    if (A > 0) {
        const int64_t An = (int64_t)A;
        const int key_bits = 2 * d.ubits;
        const size_t sort_bytes = pc_sort_temp_bytes(An, key_bits);
        if ((rc = c->b_key0.ensure(A * 8)) || (rc = c->b_key1.ensure(A * 8)) || (rc = c->b_val0.ensure(A * 4)) || (rc = c->b_val1.ensure(A * 4)) ||
            (rc = c->b_sort_tmp.ensure(std::max<size_t>(sort_bytes, 16))) || (rc = c->b_flags.ensure((A + 1) * 4)) || (rc = c->b_excl.ensure((A + 1) * 4)) ||
            (rc = c->b_alias.ensure(A * 4)) || (rc = c->b_bucket_row.ensure(A * 4)) || (rc = c->b_res.ensure(A * 8)) ||
            (rc = c->b_scan_tmp.ensure(pc_scan_tmp_elems(std::max<int64_t>(tmp_fixed, An + 1)) * 4)))
            return rc;
        const int64_t tmp_elems = (int64_t)(c->b_scan_tmp.cap / 4);
        // 2 ENUM: one sort key per alignment slot; 3 sort; 4 distinct alignments, aliases, buckets (pc_plan.hip)
        a.key = c->b_key0.as<unsigned long long>(); a.val = c->b_val0.as<uint32_t>();
        if ((rc = walk_domain(c, PCW_ENUM, dom, k0, k1, a, st))) return rc;
        if ((rc = pc_sort_pairs(c->b_sort_tmp.p, c->b_sort_tmp.cap, c->b_key0.as<unsigned long long>(), c->b_key1.as<unsigned long long>(),
                                c->b_val0.as<uint32_t>(), c->b_val1.as<uint32_t>(), An, key_bits, st))) return rc;
        if ((rc = pc_launch_mark_heads(c->b_key1.as<unsigned long long>(), c->b_flags.as<uint32_t>(), An, st))) return rc;
        if ((rc = pc_scan_exclusive_u32(c->b_flags.as<uint32_t>(), c->b_excl.as<uint32_t>(), An + 1, c->b_scan_tmp.as<uint32_t>(), tmp_elems, st))) return rc;
        PC_HIP(hipMemsetAsync(c->b_start_q.p, 0, (U + 1) * 4, st));
        PC_HIP(hipMemsetAsync(c->b_end_q.p, 0, (U + 1) * 4, st));
        PC_HIP(hipMemsetAsync(c->b_totals.as<unsigned long long>() + 3, 0, 16, st));        // distinct alignments / cells of THIS chunk
        if ((rc = pc_launch_unique(d, c->b_key1.as<unsigned long long>(), c->b_val1.as<uint32_t>(), c->b_flags.as<uint32_t>(), c->b_excl.as<uint32_t>(),
                                   c->b_alias.as<uint32_t>(), c->b_bucket_row.as<int32_t>(), c->b_start_q.as<uint32_t>(), c->b_end_q.as<uint32_t>(),
                                   c->b_totals.as<unsigned long long>(), An, st))) return rc;
        // 5 workgroup tasks per column sequence (a bucket's left-over rows may go to a narrower variant); second
        //   read-back: number of tasks, distinct totals
        if ((rc = pc_launch_task_count(c->b_start_q.as<uint32_t>(), c->b_end_q.as<uint32_t>(), c->task_plan, c->b_ntask_q.as<uint32_t>(), U, st))) return rc;
        if ((rc = pc_scan_exclusive_u32(c->b_ntask_q.as<uint32_t>(), c->b_task_off_q.as<uint32_t>(), U + 1, c->b_scan_tmp.as<uint32_t>(), tmp_elems, st))) return rc;
        PC_HIP(hipMemcpyAsync(h_plan, c->b_task_off_q.as<uint32_t>() + U, 4, hipMemcpyDeviceToHost, st));
        PC_HIP(hipMemcpyAsync(h_tot, c->b_totals.p, 40, hipMemcpyDeviceToHost, st));
        PC_HIP(hipStreamSynchronize(st));
        const uint32_t ntasks = h_plan[0];
        local.n_tasks = ntasks; local.n_distinct_alignments = (int64_t)h_tot[3]; local.n_distinct_cells = (int64_t)h_tot[4];
        P.ntasks = ntasks; P.n_distinct = (int64_t)h_tot[3];
        int cbits = 1; while ((1 << cbits) < ncls) ++cbits;
        const size_t tb_bytes = pc_sort_temp_bytes((int64_t)std::max<uint32_t>(ntasks, 1), 32 + cbits);
        if ((rc = c->b_tasks.ensure(std::max<uint32_t>(ntasks, 1) * sizeof(PcTask))) || (rc = c->b_tasks_sorted.ensure(std::max<uint32_t>(ntasks, 1) * sizeof(PcTask))) ||
            (rc = c->b_key0.ensure((size_t)ntasks * 8)) || (rc = c->b_key1.ensure((size_t)ntasks * 8)) || (rc = c->b_val0.ensure((size_t)ntasks * 4)) ||
            (rc = c->b_val1.ensure((size_t)ntasks * 4)) || (rc = c->b_sort_tmp.ensure(std::max<size_t>(tb_bytes, 16))))
            return rc;
        if ((rc = pc_launch_task_fill(d, c->b_start_q.as<uint32_t>(), c->b_end_q.as<uint32_t>(), c->task_plan,
                                      c->b_task_off_q.as<uint32_t>(), c->b_tasks.as<PcTask>(), U, st))) return rc;
        // 6 the task list sorted by (launch class, longest first) with the same radix sort (the key/value buffers of the
        //   alignment sort are free again); third read-back: task range and longest column per launch class
        if ((rc = pc_launch_task_keys(d, c->b_tasks.as<PcTask>(), c->b_key0.as<unsigned long long>(),
                                      c->b_val0.as<uint32_t>(), (int)ntasks, st))) return rc;
        if ((rc = pc_sort_pairs(c->b_sort_tmp.p, c->b_sort_tmp.cap, c->b_key0.as<unsigned long long>(), c->b_key1.as<unsigned long long>(),
                                c->b_val0.as<uint32_t>(), c->b_val1.as<uint32_t>(), (int64_t)ntasks, 32 + cbits, st))) return rc;
        if ((rc = pc_launch_task_gather(c->b_tasks.as<PcTask>(), c->b_val1.as<uint32_t>(), c->b_tasks_sorted.as<PcTask>(), (int)ntasks, st))) return rc;
        if ((rc = pc_launch_class_bounds(c->b_key1.as<unsigned long long>(), (int)ntasks, ncls, c->b_cls_begin.as<uint32_t>(), st))) return rc;
        PC_HIP(hipMemcpyAsync(h_plan, c->b_cls_begin.p, (size_t)(ncls + 1) * 4, hipMemcpyDeviceToHost, st));
        PC_HIP(hipStreamSynchronize(st));
        P.tb.assign(h_plan, h_plan + ncls + 1);
    }
    P.valid = true;
    return PC_OK;
}

// ALIGN: the K4 launches over the planned tasks -- all of them, or every world-th task of each launch class starting at
// slice_rank (tasks of a class are sorted longest first, so the slices of a class carry equal work); results go to
// res[position of the distinct alignment], entries of tasks outside the slice are left zero.
static int stage_align(pc_ctx* c, int slice_rank, int slice_world, uint2* res, hipStream_t st, pc_stats* stats) {
    PcRange range("pc:align");
    pc_ctx::PlanState& P = c->plan;
    if (!P.valid) { pc_set_error("align: no plan (pc_plan_dev first)"); return PC_ERR_STATE; }
    const int ncls = c->nlc;
    c->aligned_tasks.assign(ncls, 0);
    if (P.A <= 0 || P.ntasks == 0) return PC_OK;
    int rc = PC_OK;
    const PcTask* task_list = c->b_tasks_sorted.as<PcTask>();
    std::vector<uint32_t> tb = P.tb;
    if (slice_world > 1) {
        std::vector<uint32_t> sb(ncls + 1, 0);
        for (int i = 0; i < ncls; ++i) {
            const uint32_t n = P.tb[i + 1] - P.tb[i];
            sb[i + 1] = sb[i] + (n > (uint32_t)slice_rank ? (n - (uint32_t)slice_rank + (uint32_t)slice_world - 1) / (uint32_t)slice_world : 0u);
        }
        if ((rc = upload_vec(c->b_slice_begin, sb))) return rc;
        if ((rc = pc_launch_task_slice(task_list, (int)P.ntasks, c->b_cls_begin.as<uint32_t>(), c->b_slice_begin.as<uint32_t>(), slice_rank, slice_world,
                                       c->b_tasks.as<PcTask>(), st))) return rc;       // (b_tasks: the unsorted list, free again)
        PC_HIP(hipMemsetAsync(res, 0, (size_t)std::max<int64_t>(P.n_distinct, 1) * 8, st));
        task_list = c->b_tasks.as<PcTask>(); tb = sb;
    }
    for (int i = 0; i < ncls; ++i) c->aligned_tasks[i] = tb[i + 1] - tb[i];
    return run_align_classes(c, task_list, tb.data(), c->cls_max_lb.data(), res, st, stats, P.ppos);
}

// REDUCE: best match per anchor gene through the aliases, fp64 epilogue (metrics.py:204-232, 247-253), over the plan's targets: o's one
// metric into its array, or its joint set, each metric into its own, in one walk
static int stage_reduce(pc_ctx* c, const PcFillOut& o, int as_distance, const uint2* res, hipStream_t st, const PcUnitDomain& dom = PcUnitDomain{}) {
    PcRange range("pc:reduce");
    pc_ctx::PlanState& P = c->plan;
    if (!P.valid) { pc_set_error("reduce: no plan (pc_plan_dev first)"); return PC_ERR_STATE; }
    PcJointArgs a; memset(&a, 0, sizeof(a));
    a.off = c->b_off.as<uint32_t>(); a.alias = c->b_alias.as<uint32_t>(); a.res = res; a.out = o.out;
    a.as_distance = as_distance ? 1 : 0; a.condensed = P.condensed;
    if (!o.mask) return walk_domain(c, o.metric == PC_AAI ? PCW_AAI : PCW_PEQ, dom, P.k0, P.k1, a, st);
    a.mask = o.mask;
    for (int m = 0; m < 6; ++m) a.jout[m] = o.joint[m];
    return walk_domain_joint(c, dom, P.k0, P.k1, a, st);
}

// a finished chunk: its plan's counts, and its tasks per launch class for pc_last_plan_tasks
static void add_plan_stats(pc_ctx* c, pc_stats& acc) {
    const pc_stats& ps = c->plan.st;
    acc.n_tasks += ps.n_tasks; acc.n_distinct_alignments += ps.n_distinct_alignments; acc.n_distinct_cells += ps.n_distinct_cells;
    for (size_t i = 0; i < c->aligned_tasks.size() && i < c->last_plan_tasks.size(); ++i) c->last_plan_tasks[i] += c->aligned_tasks[i];
}
static void set_last_plan_tasks(pc_ctx* c, const std::vector<uint32_t>& per_class) {
    c->last_plan_tasks.assign(per_class.begin(), per_class.end());
    c->last_plan_tasks.resize(c->nlc, 0);
    c->last_plan_tasks_valid = true;
}

// One plan -> align -> reduce over the owned targets (or the units of dom) [k0, k1) holding A alignments, and its counts added
// to `local`.  events: ev[1] and ev[2] are recorded between the stages (ev[3] after them always); ms != NULL: the step is waited for and its
// three stage times, the first counted from `from`, are added to ms[0..2].
static int chunk_step(pc_ctx* c, const PcFillOut& o, int ppos, int as_distance, int condensed, hipStream_t st, int k0, int k1, uint64_t A,
                      const PcUnitDomain& dom, pc_stats& local, bool events, hipEvent_t from, float* ms) {
    int rc = stage_plan(c, ppos, condensed, st, k0, k1, A, dom);
    if (rc == PC_OK) { if (events) PC_HIP(hipEventRecord(c->ev[1], st)); rc = stage_align(c, 0, 1, c->b_res.as<uint2>(), st, &local); }
    if (rc == PC_OK) { if (events) PC_HIP(hipEventRecord(c->ev[2], st)); rc = stage_reduce(c, o, as_distance, c->b_res.as<uint2>(), st, dom); }
    if (rc != PC_OK) return rc;
    PC_HIP(hipEventRecord(c->ev[3], st));
    add_plan_stats(c, local);
    if (ms) {
        const hipEvent_t at[4] = {from, c->ev[1], c->ev[2], c->ev[3]};
        PC_HIP(hipEventSynchronize(c->ev[3]));
        for (int i = 0; i < 3; ++i) { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, at[i], at[i + 1])); ms[i] += x; }
    }
    return PC_OK;
}
// out of HBM in a step: free the plan (and the strip-mined launches' slab; slots: and the slot arrays of a range of units) once nothing
// reads them any more; the caller goes on with half the chunk
static int release_for_retry(pc_ctx* c, hipStream_t st, bool slots) {
    PC_HIP(hipStreamSynchronize(st));
    release_plan_buffers(c);
    c->b_scratch.release();
    if (slots) { c->b_na.release(); c->b_off.release(); }
    return PC_OK;
}

// aai / peq / a joint set: COUNT once, then plan -> align -> reduce -- in one piece when the plan fits the budget, else chunk by chunk
int fill_aligned(pc_ctx* c, const PcFillOut& o, int ppos, int as_distance, int condensed, hipStream_t st, pc_stats& local, bool timed) {
    int rc = PC_OK;
    if ((rc = fill_check_residues(c, "fill", o.metric))) return rc;
    uint64_t tot[3] = {0, 0, 0};
    c->last_plan_tasks_valid = false;
    c->last_plan_tasks.assign(c->nlc, 0);
    if ((rc = stage_count(c, condensed, st, tot))) return rc;
    local.n_alignments = (int64_t)tot[0]; local.n_cells = (int64_t)tot[1]; local.n_residue_bytes = (int64_t)tot[2];
    const int nown = c->shard.nown;
    const uint64_t A = tot[0];
    // does the whole plan fit?  (hipMemGetInfo only when the question is open: plans under 1 GiB always do)
    uint64_t max_aln = (uint64_t)PC_PLAN_MAX_ALIGNMENTS;
    if (c->plan_budget > 0 || A * PC_PLAN_BYTES_PER_ALIGNMENT > ((uint64_t)1 << 30))
        max_aln = std::min<uint64_t>(max_aln, (uint64_t)std::max<int64_t>(plan_budget_bytes(c) / PC_PLAN_BYTES_PER_ALIGNMENT, 1));
    local.n_chunks = 0;
    if (A <= max_aln) {
        // (its stage times are read by fill_impl: ev[0] .. ev[3])
        rc = chunk_step(c, o, ppos, as_distance, condensed, st, 0, nown, A, PcUnitDomain{}, local, true, nullptr, nullptr);
        if (rc == PC_OK) {
            local.n_chunks = 1;
            c->last_plan_tasks_valid = true;
            return PC_OK;
        }
        if (rc != PC_ERR_NOMEM_INTERNAL) return rc;
        if ((rc = release_for_retry(c, st, false))) return rc;            // go on in chunks of half the size
        max_aln = std::max<uint64_t>(A / 2, 1);
        local.n_tasks = 0; local.n_distinct_alignments = local.n_distinct_cells = 0; local.n_align_launches = 0;
    }
    // ---- chunked: successive ranges of the owned targets, each planned, aligned and reduced before the next
    std::vector<uint64_t> per_owned;
    if ((rc = count_per_target(c, condensed, st, per_owned))) return rc;
    float ms[3] = {0.f, 0.f, 0.f};                                        // plan, align, reduce
    int k = 0, nchunks = 0;
    while (k < nown) {
        // the next chunk: as many targets from k on as stay within max_aln (pc_chunk_plan's rule)
        uint64_t run = per_owned[k]; int k1 = k + 1;
        while (k1 < nown && run + per_owned[k1] <= max_aln) { run += per_owned[k1]; ++k1; }
        if (timed) PC_HIP(hipEventRecord(c->ev[4], st));
        rc = chunk_step(c, o, ppos, as_distance, condensed, st, k, k1, run, PcUnitDomain{}, local, timed, c->ev[4], timed ? ms : nullptr);
        if (rc == PC_ERR_NOMEM_INTERNAL && max_aln > 1 && k1 - k > 1) {                 // a retry with a smaller chunk, not an error
            if ((rc = release_for_retry(c, st, false))) return rc;
            max_aln = std::max<uint64_t>(std::min(max_aln, run) / 2, 1);
            continue;
        }
        if (rc != PC_OK) return rc;
        ++nchunks; k = k1;
    }
    c->plan.valid = false;                                                // the last chunk's plan is not "the plan of the fill"
    local.n_chunks = nchunks;
    c->last_plan_tasks_valid = true;
    local.ms_plan = ms[0]; local.ms_align = ms[1]; local.ms_reduce = ms[2];
    return PC_OK;
}

// aai / peq over a domain that is cut into UNITS -- the query rows of a rows fill (pc_fill_rows*), the row blocks of TS positions of a
// groups fill (pc_fill_groups*), the blocks of PC_PAIR_BLOCK slots of a pair-list fill (pc_fill_pairs*): COUNT over every unit (totals, alignments per unit: aln_t), then plan -> align -> reduce over successive
// ranges of units.  The ranges follow pc_chunk_plan over the units' costs under the budget a whole fill has (pc_set_plan_budget /
// PC_PLAN_BYTES, 2^31-2 alignments per plan, a failed allocation halves the range); a unit costs its alignments plus its slots of na /
// off (8 bytes each, stated in alignments), so a request of many units never holds more than a range's worth of slot arrays.  A range of
// units is a range of slots: N per query row; for row blocks block_slot[] says where (and a range of the tile list, block_tile[]); a
// block of a pair list holds PC_PAIR_BLOCK consecutive slots.  One
// plan per range merges the duplicate sequence pairs of everything the range touches.  `out` is the whole result; the reduce of a range
// writes its cells (a rows fill: also the mirror cells of pairs of two queries).  Values do not depend on the cut: every pair's
// alignments stay in one range.
static int fill_units_aligned(pc_ctx* c, const PcUnitDomain& dom, const PcFillOut& o, int ppos, int as_distance,
                              hipStream_t st, pc_stats& local, bool timed) {
    int rc = PC_OK;
    const PcDev& d = c->dev;
    const int U = dom.units();
    auto slots = [&](int k0, int k1) { return dom.slots(k0, k1, d.N); };
    if ((rc = fill_check_residues(c, "fill", o.metric))) return rc;
    if (d.G > 0 && c->min_gene_len == 0) {
        pc_set_error("fill: an empty translation cannot be aligned (aai/peq); the reference fails on it too"); return PC_ERR_DATA;
    }
    c->last_plan_tasks_valid = false;
    c->last_plan_tasks.assign(c->nlc, 0);
    c->plan.valid = false;
    // COUNT over all units: totals and alignments per unit (no slot array yet)
    std::vector<uint64_t> own(U);
    {
        PcRange range("pc:count");
        if ((rc = c->b_totals.ensure(64)) || (rc = c->b_aln_t.ensure((size_t)std::max(U, 1) * 8))) return rc;
        PC_HIP(hipMemsetAsync(c->b_totals.p, 0, 64, st));
        PC_HIP(hipMemsetAsync(c->b_aln_t.p, 0, (size_t)U * 8, st));
        PcWalkArgs a; memset(&a, 0, sizeof(a));
        a.totals = c->b_totals.as<unsigned long long>(); a.aln_t = c->b_aln_t.as<unsigned long long>();
        if ((rc = walk_domain(c, PCW_COUNT, dom, 0, U, a, st))) return rc;
        uint64_t* h_tot = (uint64_t*)(c->h_plan.as<uint32_t>() + 1000);
        PC_HIP(hipMemcpyAsync(h_tot, c->b_totals.p, 24, hipMemcpyDeviceToHost, st));
        PC_HIP(hipMemcpyAsync(own.data(), c->b_aln_t.p, (size_t)U * 8, hipMemcpyDeviceToHost, st));
        PC_HIP(hipStreamSynchronize(st));
        local.n_alignments = (int64_t)h_tot[0]; local.n_cells = (int64_t)h_tot[1]; local.n_residue_bytes = (int64_t)h_tot[2];
    }
    const uint64_t A = (uint64_t)local.n_alignments;
    // a unit's cost in alignments: its own + the 8 bytes per slot of its entries of na / off
    std::vector<uint64_t> slot_cost(U), cost(U);
    uint64_t all_slot_cost = 0;
    for (int k = 0; k < U; ++k) {
        slot_cost[k] = ((uint64_t)slots(k, k + 1) * 8 + PC_PLAN_BYTES_PER_ALIGNMENT - 1) / PC_PLAN_BYTES_PER_ALIGNMENT;
        cost[k] = own[k] + slot_cost[k];
        all_slot_cost += slot_cost[k];
    }
    uint64_t max_aln = (uint64_t)PC_PLAN_MAX_ALIGNMENTS;
    if (c->plan_budget > 0 || (A + all_slot_cost) * PC_PLAN_BYTES_PER_ALIGNMENT > ((uint64_t)1 << 30))
        max_aln = std::min<uint64_t>(max_aln, (uint64_t)std::max<int64_t>(plan_budget_bytes(c) / PC_PLAN_BYTES_PER_ALIGNMENT, 1));
    float ms[3] = {0.f, 0.f, 0.f};                                        // plan (with the range's COUNT), align, reduce
    int k = 0, nchunks = 0;
    while (k < U) {
        int32_t cut[2] = {0, 0};
        if ((rc = pc_chunk_plan(cost.data() + k, U - k, max_aln, cut, 2)) < 0) return rc;
        const int k1 = k + cut[1];
        const int64_t Lc = slots(k, k1);
        uint64_t run = 0, run_slot_cost = 0;
        for (int i = k; i < k1; ++i) { run += own[i]; run_slot_cost += slot_cost[i]; }
        if (Lc == 0) { k = k1; continue; }                                    // (row blocks of one-member groups: no slot, no tile)
        if (timed) PC_HIP(hipEventRecord(c->ev[4], st));
        // the range's own COUNT: alignments per slot (its totals go to scratch words nobody reads)
        rc = c->b_na.ensure((Lc + 1) * 4);
        if (rc == PC_OK) rc = c->b_off.ensure((Lc + 1) * 4);
        if (rc == PC_OK) {
            PC_HIP(hipMemsetAsync(c->b_na.p, 0, (Lc + 1) * 4, st));
            PcWalkArgs a; memset(&a, 0, sizeof(a));
            a.na = c->b_na.as<uint32_t>(); a.totals = c->b_totals.as<unsigned long long>() + 5;
            rc = walk_domain(c, PCW_COUNT, dom, k, k1, a, st);
        }
        if (rc == PC_OK) rc = chunk_step(c, o, ppos, as_distance, 0, st, k, k1, run, dom, local, timed, c->ev[4], timed ? ms : nullptr);
        if (rc == PC_ERR_NOMEM_INTERNAL && max_aln > 1 && k1 - k > 1) {                 // a retry with a smaller range, not an error
            if ((rc = release_for_retry(c, st, true))) return rc;
            max_aln = std::max<uint64_t>(std::min(max_aln, run + run_slot_cost) / 2, 1);
            continue;
        }
        if (rc != PC_OK) return rc;
        ++nchunks; k = k1;
    }
    c->plan.valid = false;                                                // such a plan serves no later stage
    local.n_chunks = nchunks;
    c->last_plan_tasks_valid = true;
    local.ms_plan = ms[0]; local.ms_align = ms[1]; local.ms_reduce = ms[2];
    return PC_OK;
}

// a rows fill (the units are the query rows), a groups fill (the row blocks of TS positions) or a pair-list fill (the blocks of
// PC_PAIR_BLOCK slots), every metric: the set metrics always run on the domain's walker, all units in one launch (no selector:
// pc_last_set_kernel / pc_last_set_launch keep reporting the last whole fill)
int fill_units(pc_ctx* c, const PcUnitDomain& dom, const PcFillOut& o, int ppos, int as_distance, hipStream_t st, pc_stats& local, bool timed) {
    const int metric = o.metric;
    if (o.mask || metric >= PC_AAI) return fill_units_aligned(c, dom, o, ppos, as_distance, st, local, timed);
    PcWalkArgs a; memset(&a, 0, sizeof(a));
    a.out = o.out; a.as_distance = as_distance;
    const int mode = metric == PC_GCS ? PCW_GCS : metric == PC_JC ? PCW_JC : metric == PC_POCP ? PCW_POCP : PCW_AF;
    return walk_domain(c, mode, dom, 0, dom.units(), a, st);
}

// ---- alignment-sliced multi-GPU route (aai / peq): every rank plans the whole (unsharded) fill -- milliseconds --, aligns
// every world-th task of each launch class, the per-alignment results are summed to the root (entries of foreign tasks are
// zero), and the root reduces.  Each distinct (row sequence, column sequence) pair is then aligned once in the whole JOB,
// not once per rank, and the ranks carry equal work by construction (no cost-balanced deal, no COUNT pass for it).
extern "C" int pc_plan_dev(pc_ctx* c, int metric, void* stream, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_plan_dev: upload first"); return PC_ERR_STATE; }
    if (metric != PC_AAI && metric != PC_PEQ && metric != PC_AAI_PPOS) { pc_set_error("pc_plan_dev: metric %d has no alignment plan", metric); return PC_ERR_ARG; }
    if (c->world != 1) { pc_set_error("pc_plan_dev: context is sharded (%d/%d); the alignment-sliced route plans the whole matrix", c->rank, c->world); return PC_ERR_STATE; }
    if (!c->residues_ready) { pc_set_error("pc_plan_dev: the residues are not on the device (pc_upload_residues)"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    int rc = wait_last_work(c, st, true); if (rc != PC_OK) return rc;
    PC_HIP(hipEventRecord(c->ev[0], st));
    uint64_t tot[3] = {0, 0, 0};
    if ((rc = stage_count(c, 1, st, tot))) return abi_rc(rc);
    if (tot[0] > (uint64_t)PC_PLAN_MAX_ALIGNMENTS) {
        pc_set_error("pc_plan_dev: %llu alignments exceed the 2^31-2 one plan can index; the alignment-sliced route keeps the whole plan resident "
                     "-- use the pair-sharded route (pc_fill_shard_dev), which fills in chunks", (unsigned long long)tot[0]);
        return PC_ERR_LIMIT;
    }
    rc = stage_plan(c, metric == PC_AAI_PPOS, 1, st, 0, c->shard.nown, tot[0]);
    (void)mark_work(c, st);
    if (rc != PC_OK) return abi_rc(rc);
    c->plan.st.n_cells = (int64_t)tot[1]; c->plan.st.n_residue_bytes = (int64_t)tot[2];
    {   // pc_last_plan_tasks: the whole plan's tasks per launch class, until a slice of it is aligned
        std::vector<uint32_t> per_class(c->nlc, 0);
        for (int i = 0; i < c->nlc; ++i) per_class[i] = c->plan.tb[i + 1] - c->plan.tb[i];
        set_last_plan_tasks(c, per_class);
    }
    PC_HIP(hipEventRecord(c->ev[1], st));
    if ((rc = mark_work(c, st))) return rc;
    if (stats) {
        PC_HIP(hipEventSynchronize(c->ev[1]));
        c->busy = false;
        *stats = c->plan.st;
        stats->n_chunks = 1;
        PC_HIP(hipEventElapsedTime(&stats->ms_plan, c->ev[0], c->ev[1]));
        stats->ms_total = stats->ms_plan;
    }
    return PC_OK;
}

extern "C" int pc_align_slice_dev(pc_ctx* c, int slice_rank, int slice_world, void* res_dev, void* stream, pc_stats* stats) {
    if (!c || !c->uploaded || !c->plan.valid) { pc_set_error("pc_align_slice_dev: pc_plan_dev first"); return PC_ERR_STATE; }
    if (!c->plan.whole) { pc_set_error("pc_align_slice_dev: the plan in the context is not a whole-matrix plan of an unsharded context (pc_plan_dev)"); return PC_ERR_STATE; }
    if (slice_world < 1 || slice_rank < 0 || slice_rank >= slice_world) { pc_set_error("pc_align_slice_dev: slice %d of %d", slice_rank, slice_world); return PC_ERR_ARG; }
    if (!res_dev && c->plan.n_distinct > 0) { pc_set_error("pc_align_slice_dev: res_dev is NULL"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    // a slice still running on ANOTHER stream reads the task tables this call rewrites
    int rc = wait_last_work(c, st, true); if (rc != PC_OK) return rc;
    pc_stats local = c->plan.st;
    PC_HIP(hipEventRecord(c->ev[1], st));
    rc = stage_align(c, slice_rank, slice_world, (uint2*)res_dev, st, &local);
    if (rc == PC_OK) set_last_plan_tasks(c, c->aligned_tasks);           // this slice's own counts
    PC_HIP(hipEventRecord(c->ev[2], st));
    int rc2 = mark_work(c, st);
    if (rc != PC_OK) return abi_rc(rc);
    if (rc2 != PC_OK) return rc2;
    if (stats) {
        PC_HIP(hipEventSynchronize(c->ev[2]));
        c->busy = false;
        PC_HIP(hipEventElapsedTime(&local.ms_align, c->ev[1], c->ev[2]));
        local.ms_total = local.ms_align;
        local.n_chunks = 1;
        *stats = local;
    }
    return PC_OK;
}

extern "C" int pc_reduce_dev(pc_ctx* c, int metric, int as_distance, const void* res_dev, void* out_condensed_dev, void* stream) {
    if (!c || !c->uploaded || !c->plan.valid) { pc_set_error("pc_reduce_dev: pc_plan_dev first"); return PC_ERR_STATE; }
    if (!c->plan.whole) { pc_set_error("pc_reduce_dev: the plan in the context is not a whole-matrix plan of an unsharded context (pc_plan_dev)"); return PC_ERR_STATE; }
    if (metric == PC_AAI_PPOS) metric = PC_AAI;
    if (metric != PC_AAI && metric != PC_PEQ) { pc_set_error("pc_reduce_dev: metric %d", metric); return PC_ERR_ARG; }
    if (!out_condensed_dev || (!res_dev && c->plan.n_distinct > 0)) { pc_set_error("pc_reduce_dev: NULL argument"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    int rc = wait_last_work(c, st, true); if (rc != PC_OK) return rc;
    rc = stage_reduce(c, PcFillOut(metric, (double*)out_condensed_dev), as_distance, (const uint2*)res_dev, st);
    int rc2 = mark_work(c, st);
    return rc != PC_OK ? abi_rc(rc) : rc2;
}

extern "C" int pc_align_pairs(pc_ctx* c, const int32_t* a_gene, const int32_t* b_gene, int64_t n, int variant,
                              int32_t* n_ident, int32_t* n_diag) {
    if (!c || !c->uploaded) { pc_set_error("pc_align_pairs: upload first"); return PC_ERR_STATE; }
    if (n < 0 || (n > 0 && (!a_gene || !b_gene || !n_ident || !n_diag))) { pc_set_error("pc_align_pairs: NULL argument"); return PC_ERR_ARG; }
    if (n == 0) return PC_OK;
    if (n >= 0x7fffffffLL) { pc_set_error("pc_align_pairs: too many pairs"); return PC_ERR_LIMIT; }
    if (!c->residues_ready) { pc_set_error("pc_align_pairs: the residues are not on the device (pc_upload_residues)"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    int rc = wait_last_work(c, nullptr, false); if (rc != PC_OK) return rc;
    c->plan.valid = false;                             // this call reuses the plan's task, bucket and result buffers
    const int G = c->dev.G;
    const int nvar = pc_nw_num_variants();
    int forced = -2;                                   // -2: automatic
    const bool like_fill = variant >= 1000;            // 1000 + w: variant w, its buckets cut as a fill cuts them (tools/class_rates.py)
    if (like_fill) variant -= 1000;
    if (variant < 0) forced = -1;
    else if (variant > 0) {
        for (int v = 0; v < nvar; ++v) if (pc_nw_variant_w(v) == variant) forced = v;
        if (forced == -2) { pc_set_error("pc_align_pairs: no systolic variant with %d columns per lane", variant); return PC_ERR_ARG; }
    }
    std::vector<int> cls(n);
    std::vector<int32_t> sums(n);
    for (int64_t k = 0; k < n; ++k) {
        if (a_gene[k] < 0 || a_gene[k] >= G || b_gene[k] < 0 || b_gene[k] >= G) { pc_set_error("pc_align_pairs: gene index out of range at %lld", (long long)k); return PC_ERR_ARG; }
        const int la = c->h_gene_len[a_gene[k]], lb = c->h_gene_len[b_gene[k]];
        if (la == 0 || lb == 0) { pc_set_error("pc_align_pairs: empty translation at %lld", (long long)k); return PC_ERR_DATA; }
        int v = forced == -2 ? pc_nw_choose_variant(lb) : forced;
        if (v >= 0 && lb > 64 * pc_nw_variant_w(v) && pc_nw_variant_w(v) < 32) { pc_set_error("pc_align_pairs: column gene of %d residues does not fit variant w=%d (strip-mined passes exist for w = 32, 48, 64)", lb, pc_nw_variant_w(v)); return PC_ERR_ARG; }
        cls[k] = pc_class_of(lb, v, c->h_gene_odd[b_gene[k]] != 0);                           // as pc_upload classes such column genes
        sums[k] = la + lb;
    }
    std::vector<int64_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        if (cls[x] != cls[y]) return cls[x] < cls[y];
        if (b_gene[x] != b_gene[y]) return b_gene[x] < b_gene[y];
        return x < y;
    });
    std::vector<int32_t> rows(n); std::vector<uint32_t> dest(n); std::vector<PcTask> tasks;
    const int nlc = pc_num_classes() * PC_WAVE_MODES;
    std::vector<uint32_t> cls_task_begin(nlc + 1, 0);
    std::vector<int> cls_maxlb(nlc, 0);
    {
        // Buckets (runs of one column gene) are cut the way the fill's planner cuts them (pc_plan.hip): tasks of the class's row
        // count; with the automatic variant also the left-over rows of a wave round to the remainder chooser's variant, and every
        // task in the launch mode its row count asks for.  A forced variant keeps its class's own workgroup shape (unless asked as 1000 + w).
        for (int64_t i = 0; i < n;) {
            const int64_t k = order[i];
            int64_t j = i;
            while (j < n && cls[order[j]] == cls[k] && b_gene[order[j]] == b_gene[k]) ++j;
            const int lb = c->h_gene_len[b_gene[k]];
            const bool odd = c->h_gene_odd[b_gene[k]] != 0;
            const PcBucketCut cut = pc_bucket_cut(lb, j - i, cls[k], odd, forced == -2 || like_fill);
            const int per = cut.per, rem_cls = cut.rem_base;
            const int64_t jmain = i + cut.n_main;
            auto put = [&](int64_t r0, int64_t r1, int base) {
                PcTask t; t.gene = b_gene[k]; t.begin = (int32_t)r0; t.end = (int32_t)r1;
                t.pad = pc_task_launch_class(lb, (int)(r1 - r0), base, forced == -2 || like_fill);
                cls_maxlb[t.pad] = std::max(cls_maxlb[t.pad], lb);
                tasks.push_back(t);
            };
            for (int64_t r = i; r < jmain; r += per) put(r, std::min<int64_t>(jmain, r + per), cls[k]);
            if (rem_cls >= 0) put(jmain, j, rem_cls);
            for (int64_t r = i; r < j; ++r) { rows[r] = a_gene[order[r]]; dest[r] = (uint32_t)order[r]; }
            i = j;
        }
        // By launch class, longest tasks first inside a class, as pc_fill's plan orders them.  Workgroups go to the 8 XCDs
        // round-robin by block index, so a list that alternates full tasks and left-overs (every bucket cut the same way) puts
        // all the full ones on half of the XCDs: measured 2x the time on uniform test data.
        std::stable_sort(tasks.begin(), tasks.end(), [&](const PcTask& x, const PcTask& y) {
            if (x.pad != y.pad) return x.pad < y.pad;
            const int64_t wx = (int64_t)(x.end - x.begin) * c->h_gene_len[x.gene], wy = (int64_t)(y.end - y.begin) * c->h_gene_len[y.gene];
            return wx > wy;
        });
        size_t at = 0;
        for (int lc = 0; lc <= nlc; ++lc) { while (at < tasks.size() && tasks[at].pad < lc) ++at; cls_task_begin[lc] = (uint32_t)at; }
    }
    DevBuf d_sums, d_ident, d_diag;                    // (freed on every way out of this call)
    hipStream_t st = c->stream;
    if ((rc = upload_vec(c->b_bucket_row, rows)) || (rc = upload_vec(c->b_bucket_dest, dest)) || (rc = upload_vec(c->b_tasks, tasks)) ||
        (rc = c->b_res.ensure(n * 8)) || (rc = upload_vec(d_sums, sums)) || (rc = d_ident.ensure(n * 4)) || (rc = d_diag.ensure(n * 4))) return abi_rc(rc);
    (void)hipEventRecord(c->ev[1], st);
    for (int lc = 0; lc < nlc; ++lc) {
        const int nt = (int)(cls_task_begin[lc + 1] - cls_task_begin[lc]);
        if (nt <= 0) continue;
        void* scratch = nullptr; size_t sbytes = 0;
        const int base = lc / PC_WAVE_MODES, v = pc_class_variant(base);
        if (v < 0 || pc_nw_launch_is_strip(v, cls_maxlb[lc], lc % PC_WAVE_MODES, 0)) {
            sbytes = v < 0 ? pc_nw_fallback_scratch_bytes(cls_maxlb[lc]) : pc_nw_strip_scratch_bytes(c->max_gene_len, c->n_cu);
            if ((rc = c->b_scratch.ensure(sbytes))) return abi_rc(rc);
            scratch = c->b_scratch.p; sbytes = c->b_scratch.cap;
        }
        rc = pc_launch_nw(v, c->dev, c->b_tasks.as<PcTask>() + cls_task_begin[lc], nt, c->b_bucket_row.as<int32_t>(),
                          c->b_bucket_dest.as<uint32_t>(), c->b_res.as<uint2>(), scratch, sbytes, cls_maxlb[lc], 0, c->tie_rule, pc_class_compare_only(base), st,
                          lc % PC_WAVE_MODES, c->max_gene_len);
        if (rc != PC_OK) return rc;
    }
    (void)hipEventRecord(c->ev[2], st);
    rc = pc_launch_unpack_res(c->b_res.as<uint2>(), d_sums.as<int32_t>(), d_ident.as<int32_t>(), d_diag.as<int32_t>(), n, st);
    if (rc == PC_OK) {
        hipError_t e = hipMemcpyAsync(n_ident, d_ident.p, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_diag, d_diag.p, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipEventElapsedTime(&c->last_align_ms, c->ev[1], c->ev[2]);
        if (e != hipSuccess) { pc_set_error("pc_align_pairs: %s", hipGetErrorString(e)); rc = PC_ERR_HIP; }
    }
    return rc;
}
