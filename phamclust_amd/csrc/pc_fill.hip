// pc_fill.hip -- the fill entry points of libphamclust_hip.so over the whole matrix or shard (pc_fill, pc_fill_borrow, pc_fill_dev,
// pc_fill_shard_dev, pc_assemble_dev) and over the rows, groups and pairs domains (pc_fill_rows, pc_fill_rows_dev, pc_fill_groups,
// pc_fill_groups_dev, pc_fill_pairs, pc_fill_pairs_dev), and the joint fills (pc_fill_joint, pc_fill_joint_dev, pc_fill_pairs_joint,
// pc_fill_pairs_joint_dev: several metrics off one alignment pass): the frame they share, and pick_set_kernel, which gathers the selector's inputs from the context (the selector itself:
// pc_set_shape.hip).  The slab walks pc_fill_edges / pc_fill_components: pc_fill_slabs.hip.
#include "pc_host.h"

extern "C" int pc_last_set_launch(const pc_ctx* c, pc_set_inputs* in, pc_set_shape* shape) {
    if (!c) { pc_set_error("pc_last_set_launch: NULL context"); return PC_ERR_ARG; }
    if (c->last_set_kernel < 0) { pc_set_error("pc_last_set_launch: no gcs / jc / pocp / af fill on this context yet"); return PC_ERR_STATE; }
    if (in) *in = c->last_set_inputs;
    if (shape) *shape = c->last_set_shape;
    return PC_OK;
}

static int pick_set_kernel(pc_ctx* c, int metric) {
    pc_set_inputs in; memset(&in, 0, sizeof(in));
    in.n = c->dev.N; in.nown = c->shard.nown; in.words = c->dev.Wb; in.two_holder = c->two_holder;
    in.avg_shared = c->avg_shared; in.max_nph = c->max_nph; in.max_ngen = c->max_ngen; in.min_gene_len = c->min_gene_len;
    in.max_ent_len = c->max_ent_len; in.max_tlen = c->max_tlen; in.metric = metric; in.forced = -1;
    in.max_block_entries = pc_set_max_block_entries(c->h_sp_n.data(), c->h_owned.data(), (int64_t)c->h_owned.size());     // THIS rank's targets (k_sparse_col's value table)
    if (const char* set_force = getenv("PC_SET_KERNEL")) {             // (read per fill: the tests switch it between launches)
        static const char* const names[] = {"popc", "sparse", "sparse64", "walker", "sparsecol"};
        for (int k = 0; k < 5; ++k) if (!strcmp(set_force, names[k])) in.forced = k;
    }
    c->last_set_inputs = in;
    return pc_set_choice(in);
}

// gcs / jc / pocp on the popcount tiles.  Their epilogue table: gcs / jc over (shared, nph_s + nph_t), at most (max_nph+1) x
// (2 max_nph+1) doubles; pocp over (conserved, ngen_s + ngen_t), (2 max_ngen+1)^2; skipped when huge.  It depends on (metric,
// as_distance, that maximum) only, so it is rebuilt only when one of them changes.
static int launch_popc(pc_ctx* c, int metric, int as_distance, double* out, int condensed, hipStream_t st) {
    const int top = metric == PC_POCP ? c->max_ngen : c->max_nph;
    int sh_dim, tot_dim;
    double* lut = nullptr; bool build_lut = false; int64_t lut_key_now = -1;
    if (pc_set_table_dims(metric, top, &sh_dim, &tot_dim)) {
        if (const int rc = c->b_lut.ensure((size_t)sh_dim * tot_dim * 8)) return abi_rc(rc);
        lut = c->b_lut.as<double>();
        lut_key_now = ((int64_t)metric << 40) | ((int64_t)as_distance << 32) | (int64_t)top;
        build_lut = lut_key_now != c->lut_key || lut != c->lut_ptr;
    }
    const int rc = pc_launch_set_popc(c->dev, c->shard, metric, as_distance, out, condensed, lut, build_lut, top, st, &c->last_set_shape);
    if (rc != PC_OK) { c->lut_key = -1; c->lut_ptr = nullptr; return rc; }           // (whatever the table holds now, it is not trusted)
    if (lut) { c->lut_key = lut_key_now; c->lut_ptr = lut; }                          // remembered only once its build was launched
    return PC_OK;
}

// The close of every fill, after its launches (rc: what they returned).  A set metric ran as one launch, whose end becomes ev[3]; the
// aligned routes record ev[3] themselves, and what they queued before a failure is still marked as work in flight.  With stats the fill is
// waited for.  piece_times: a whole fill that ran in one piece left its stage boundaries in ev[1], ev[2] (fill_aligned); every chunked
// route has summed its stage times into `local` already.
static int fill_close(pc_ctx* c, int metric, hipStream_t st, int rc, pc_stats& local, pc_stats* stats, bool piece_times) {
    if (metric < PC_AAI) {
        if (rc != PC_OK) return rc;
        PC_HIP(hipEventRecord(c->ev[3], st));
        local.n_chunks = 1;
    } else if (rc != PC_OK) { (void)mark_work(c, st); return abi_rc(rc); }
    if ((rc = mark_work(c, st))) return rc;
    if (stats) {
        PC_HIP(hipEventSynchronize(c->ev[3]));
        c->busy = false;
        PC_HIP(hipEventElapsedTime(&local.ms_total, c->ev[0], c->ev[3]));
        if (metric < PC_AAI) local.ms_reduce = local.ms_total;
        else if (piece_times && local.n_chunks == 1) {
            PC_HIP(hipEventElapsedTime(&local.ms_plan, c->ev[0], c->ev[1]));
            PC_HIP(hipEventElapsedTime(&local.ms_align, c->ev[1], c->ev[2]));
            PC_HIP(hipEventElapsedTime(&local.ms_reduce, c->ev[2], c->ev[3]));
        }
        *stats = local;
    }
    return PC_OK;
}

int fill_impl(pc_ctx* c, int metric, int as_distance, double* out, int condensed, hipStream_t st, pc_stats* stats) {
    int ppos = 0, rc = PC_OK;
    if ((rc = fill_check(c, "fill", nullptr, &metric, &ppos))) return rc;
    if (!out) { pc_set_error("fill: out is NULL"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    static const char* const fill_names[] = {"pc:fill:gcs", "pc:fill:jc", "pc:fill:pocp", "pc:fill:af", "pc:fill:aai", "pc:fill:peq"};
    PcRange range(fill_names[metric]);
    // st == NULL is HIP's legacy default stream, used as such: a caller whose producers / consumers run on it (PyTorch's
    // default stream has handle 0) is ordered with these launches; the library's own streams are non-blocking
    if ((rc = wait_last_work(c, st, true))) return rc;
    const PcDev& d = c->dev;
    pc_stats local; memset(&local, 0, sizeof(local));
    local.n_pairs = c->shard_pairs;
    as_distance = as_distance ? 1 : 0;
    PC_HIP(hipEventRecord(c->ev[0], st));
    if (metric < PC_AAI) {
        const int kernel = pick_set_kernel(c, metric);
        const int mode = metric == PC_GCS ? PCW_SPARSE_GCS : metric == PC_JC ? PCW_SPARSE_JC : metric == PC_POCP ? PCW_POCP : PCW_AF;
        c->last_set_kernel = kernel;
        pc_set_shape* const shp = &c->last_set_shape;                      // (pc_last_set_launch)
        if (kernel == K_SPARSE_COL) rc = pc_launch_sparse_col(mode, d, c->shard, out, as_distance, condensed, st, shp);
        else if (kernel == K_SPARSE64) rc = pc_launch_sparse64(mode, d, c->shard, out, as_distance, condensed, st, shp);
        else if (kernel == K_POPC) rc = launch_popc(c, metric, as_distance, out, condensed, st);
        else if (kernel == K_SPARSE32) rc = pc_launch_sparse(mode, d, c->shard, out, as_distance, condensed, st, shp);
        else {                                                             // K_WALKER
            PcWalkArgs a; memset(&a, 0, sizeof(a));
            a.out = out; a.as_distance = as_distance; a.condensed = condensed;
            rc = pc_launch_walk(mode, d, c->shard, a, st, shp);
        }
    } else rc = fill_aligned(c, PcFillOut(metric, out), ppos, as_distance, condensed, st, local, stats != nullptr);
    return fill_close(c, metric, st, rc, local, stats, true);
}

extern "C" int pc_fill_dev(pc_ctx* c, int metric, int as_distance, void* out_dev, void* stream, pc_stats* stats) {
    if (c && c->uploaded && c->world != 1) { pc_set_error("pc_fill_dev: context is sharded (%d/%d); use pc_fill_shard_dev", c->rank, c->world); return PC_ERR_STATE; }
    return fill_impl(c, metric, as_distance, (double*)out_dev, 1, (hipStream_t)stream, stats);
}

// The host forms of the fills: b_out sized for the call's n doubles, the device form run into it on the context's stream, the n doubles
// copied to `host`, the stream drained.  wait: the rows and groups forms, whose device forms wait only after b_out is sized -- it may
// still be read by a fill left on another stream.
template <class Fill> static int fill_to_host(pc_ctx* c, int64_t n, void* host, bool wait, Fill fill_dev) {
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    if (wait && (rc = wait_last_work(c, c->stream, false))) return rc;
    if ((rc = c->b_out.ensure(std::max<int64_t>(n, 1) * 8))) return abi_rc(rc);
    if ((rc = fill_dev(c->b_out.p, c->stream))) return rc;
    if (n > 0) PC_HIP(hipMemcpyAsync(host, c->b_out.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    c->busy = false;
    return PC_OK;
}

extern "C" int pc_fill(pc_ctx* c, int metric, int as_distance, double* out_condensed, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill: upload first"); return PC_ERR_STATE; }
    if (!out_condensed) { pc_set_error("pc_fill: out is NULL"); return PC_ERR_ARG; }
    return fill_to_host(c, (int64_t)c->dev.N * (c->dev.N - 1) / 2, out_condensed, false,
                        [&](void* out_dev, void* st) { return pc_fill_dev(c, metric, as_distance, out_dev, st, stats); });
}

// Whole matrix into page-locked host memory that the CONTEXT owns: the D2H copy of an N = 20,000 matrix (1.6 GB) runs at
// PCIe speed (~30 ms) instead of through pageable staging (~165 ms), and the 1.6 GB are pinned once, not per call.
// *out_host stays valid until the next fill / upload on this context or its destruction.
extern "C" int pc_fill_borrow(pc_ctx* c, int metric, int as_distance, const double** out_host, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_borrow: upload first"); return PC_ERR_STATE; }
    if (!out_host) { pc_set_error("pc_fill_borrow: out_host is NULL"); return PC_ERR_ARG; }
    *out_host = nullptr;
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    const int64_t np = (int64_t)c->dev.N * (c->dev.N - 1) / 2;
    if ((rc = c->h_out.ensure((size_t)std::max<int64_t>(np, 1) * 8))) return rc;
    if ((rc = fill_to_host(c, np, c->h_out.p, false, [&](void* out_dev, void* st) { return pc_fill_dev(c, metric, as_distance, out_dev, st, stats); }))) return rc;
    *out_host = c->h_out.as<double>();
    return PC_OK;
}

extern "C" int pc_fill_shard_dev(pc_ctx* c, int metric, int as_distance, void* shard_dev, void* stream, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_shard_dev: upload first"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    if (c->shard_stride > c->shard_pairs)
        PC_HIP(hipMemsetAsync((double*)shard_dev + c->shard_pairs, 0, (c->shard_stride - c->shard_pairs) * 8, st));
    return fill_impl(c, metric, as_distance, (double*)shard_dev, 0, st, stats);
}

// ---- the domain fills: pairs of a domain other than the shard's -- the query rows of a rows fill, the within-group pairs of a groups
// fill, the listed pairs of a pair-list fill -- on an unsharded context.  Their entry points open with fill_check, validate the domain, and hand the rest to fill_domain: the
// residues check, the wait for whatever may still read the domain's device tables (upload_tables rewrites them by blocking copies and
// leaves the device view in what dom points to), fill_units, the close.  local: zeroed but for n_pairs.
template <class Tables>
static int fill_domain(pc_ctx* c, const char* who, const char* const* range_names, const PcUnitDomain& dom, int metric, int ppos,
                       int as_distance, void* out_dev, void* stream, pc_stats& local, pc_stats* stats, Tables upload_tables) {
    int rc = PC_OK;
    if ((rc = fill_check_residues(c, who, metric))) return rc;
    PC_ON_DEVICE(c);
    PcRange range(range_names[metric]);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = wait_last_work(c, st, false))) return rc;
    if ((rc = upload_tables())) return rc;
    PC_HIP(hipEventRecord(c->ev[0], st));
    rc = fill_units(c, dom, PcFillOut(metric, (double*)out_dev), ppos, as_distance ? 1 : 0, st, local, stats != nullptr);
    return fill_close(c, metric, st, rc, local, stats, false);
}

// ---- rows fill: the query genomes rows[0..n_rows) against every other genome, f64[n_rows][N]
extern "C" int pc_fill_rows_dev(pc_ctx* c, int metric, int as_distance, const int32_t* rows, int n_rows, void* out_dev, void* stream, pc_stats* stats) {
    int ppos = 0, rc = PC_OK;
    if ((rc = fill_check(c, "pc_fill_rows", "a rows fill", &metric, &ppos))) return rc;
    if (n_rows < 0) { pc_set_error("pc_fill_rows: n_rows %d", n_rows); return PC_ERR_ARG; }
    pc_stats local; memset(&local, 0, sizeof(local));
    if (n_rows == 0) { if (stats) *stats = local; return PC_OK; }
    if (!rows || !out_dev) { pc_set_error("pc_fill_rows: %s is NULL", rows ? "out" : "rows"); return PC_ERR_ARG; }
    const int N = c->dev.N;
    for (int k = 0; k < n_rows; ++k)
        if (rows[k] < 0 || rows[k] >= N || (k > 0 && rows[k] <= rows[k - 1])) {
            pc_set_error("pc_fill_rows: rows must be strictly ascending genome indices below %d (rows[%d] = %d)", N, k, rows[k]); return PC_ERR_ARG;
        }
    local.n_pairs = (int64_t)n_rows * (N - 1) - (int64_t)n_rows * (n_rows - 1) / 2;
    static const char* const fill_names[] = {"pc:fill_rows:gcs", "pc:fill_rows:jc", "pc:fill_rows:pocp", "pc:fill_rows:af", "pc:fill_rows:aai", "pc:fill_rows:peq"};
    PcRows rw{};
    PcUnitDomain dom; dom.rows = &rw;
    return fill_domain(c, "pc_fill_rows", fill_names, dom, metric, ppos, as_distance, out_dev, stream, local, stats, [&]() -> int {
        std::vector<int32_t> h_rows(rows, rows + n_rows), h_row_of((size_t)N, -1);
        for (int k = 0; k < n_rows; ++k) h_row_of[rows[k]] = k;
        int rc = PC_OK;
        if ((rc = upload_vec(c->b_rows, h_rows)) || (rc = upload_vec(c->b_row_of, h_row_of))) return rc;
        rw = PcRows{n_rows, c->b_rows.as<int32_t>(), c->b_row_of.as<int32_t>()};
        return PC_OK;
    });
}

extern "C" int pc_fill_rows(pc_ctx* c, int metric, int as_distance, const int32_t* rows, int n_rows, double* out_host, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_rows: upload first"); return PC_ERR_STATE; }
    if (n_rows > 0 && !out_host) { pc_set_error("pc_fill_rows: out is NULL"); return PC_ERR_ARG; }
    return fill_to_host(c, (int64_t)std::max(n_rows, 0) * c->dev.N, out_host, true,
                        [&](void* out_dev, void* st) { return pc_fill_rows_dev(c, metric, as_distance, rows, n_rows, out_dev, st, stats); });
}

// ---- groups fill: every pair (s, t), s < t, of two genomes in the same group of a caller-given family of groups, as the groups'
// condensed triangles end to end, f64[L].  members[M]: genome indices group by group, strictly ascending inside a group (position
// order = index order, so every pair keeps the whole fill's orientation); group_off[G+1]: each group's range.  Groups may share
// genomes; a group of 0 or 1 members has no pair.

// Host arithmetic, exported for tests: pair_off[c] = sum over c' < c of n_c' (n_c' - 1) / 2; returns L = pair_off[n_groups].
extern "C" int64_t pc_group_pair_offsets(const int64_t* group_off, int n_groups, int64_t* pair_off) {
    if (n_groups < 0 || (n_groups > 0 && !group_off)) { pc_set_error("pc_group_pair_offsets: bad argument"); return PC_ERR_ARG; }
    if (n_groups > 0 && group_off[0] != 0) { pc_set_error("pc_group_pair_offsets: group_off[0] = %lld, not 0", (long long)group_off[0]); return PC_ERR_ARG; }
    int64_t L = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t n = group_off[g + 1] - group_off[g];
        if (n < 0) { pc_set_error("pc_group_pair_offsets: group_off decreases at group %d", g); return PC_ERR_ARG; }
        if (pair_off) pair_off[g] = L;
        L += n * (n - 1) / 2;
    }
    if (pair_off) pair_off[n_groups] = L;
    return L;
}

// Per row block of PC_GROUP_TILE positions the live column blocks: a contiguous range [lo, hi] (or none).  A position p with a later member in
// its group reaches the columns p + 1 .. end - 1; only the LAST group that starts in a block can leave it, every other interval lies
// inside the block, so the union of the blocks the intervals touch has no gap.
static void group_block_ranges(const int64_t* group_off, int n_groups, int64_t M, std::vector<int32_t>& lo, std::vector<int32_t>& hi) {
    const int64_t B = (M + PC_GROUP_TILE - 1) / PC_GROUP_TILE;
    lo.assign((size_t)B, INT32_MAX); hi.assign((size_t)B, -1);
    for (int g = 0; g < n_groups; ++g) {
        const int64_t b = group_off[g], e = group_off[g + 1];
        if (e - b < 2) continue;
        const int32_t last = (int32_t)((e - 1) / PC_GROUP_TILE);
        for (int64_t a = b / PC_GROUP_TILE; a <= (e - 2) / PC_GROUP_TILE; ++a) {               // row blocks holding a position p in [b, e - 2]
            const int64_t p_first = std::max(b, a * PC_GROUP_TILE);                  // its first such p reaches column p + 1 first
            lo[a] = std::min(lo[a], (int32_t)((p_first + 1) / PC_GROUP_TILE));
            hi[a] = std::max(hi[a], last);
        }
    }
}

// Host arithmetic, exported for tests: the live tiles (row block a, column block b), a <= b, sorted by a, then b: some slot (p, q),
// p < q, both of one group, has p in block a and q in block b.  At most cap entries are written; returns their number T.
extern "C" int64_t pc_group_tiles(const int64_t* group_off, int n_groups, int32_t* tile_row, int32_t* tile_col, int64_t cap) {
    const int64_t L = pc_group_pair_offsets(group_off, n_groups, nullptr);
    if (L < 0) return L;
    const int64_t M = n_groups > 0 ? group_off[n_groups] : 0;
    if (M > 0x7fffffffLL) { pc_set_error("pc_group_tiles: %lld members exceed 2^31-1", (long long)M); return PC_ERR_ARG; }
    std::vector<int32_t> lo, hi;
    group_block_ranges(group_off, n_groups, M, lo, hi);
    int64_t T = 0;
    for (size_t a = 0; a < lo.size(); ++a)
        for (int32_t b = lo[a]; b <= hi[a]; ++b, ++T)
            if (T < cap) { if (tile_row) tile_row[T] = (int32_t)a; if (tile_col) tile_col[T] = b; }
    return T;
}

extern "C" int pc_fill_groups_dev(pc_ctx* c, int metric, int as_distance, const int32_t* members, const int64_t* group_off, int n_groups,
                                  void* out_dev, void* stream, pc_stats* stats) {
    int ppos = 0, rc = PC_OK;
    if ((rc = fill_check(c, "pc_fill_groups", "a groups fill", &metric, &ppos))) return rc;
    if (n_groups < 0) { pc_set_error("pc_fill_groups: n_groups %d", n_groups); return PC_ERR_ARG; }
    pc_stats local; memset(&local, 0, sizeof(local));
    if (n_groups == 0) { if (stats) *stats = local; return PC_OK; }
    if (!group_off) { pc_set_error("pc_fill_groups: group_off is NULL"); return PC_ERR_ARG; }
    const int64_t L = pc_group_pair_offsets(group_off, n_groups, nullptr);
    if (L < 0) return (int)L;
    const int64_t M = group_off[n_groups];
    if (M > 0x7fffffffLL) { pc_set_error("pc_fill_groups: %lld members exceed 2^31-1", (long long)M); return PC_ERR_ARG; }
    if (M > 0 && !members) {
        if (L == 0) { if (stats) *stats = local; return PC_OK; }
        pc_set_error("pc_fill_groups: members is NULL"); return PC_ERR_ARG;
    }
    const int N = c->dev.N;
    for (int g = 0; g < n_groups; ++g)
        for (int64_t p = group_off[g]; p < group_off[g + 1]; ++p)
            if (members[p] < 0 || members[p] >= N || (p > group_off[g] && members[p] <= members[p - 1])) {
                pc_set_error("pc_fill_groups: a group's members must be strictly ascending genome indices below %d (group %d, members[%lld] = %d)",
                             N, g, (long long)p, members[p]);
                return PC_ERR_ARG;
            }
    if (L == 0) { if (stats) *stats = local; return PC_OK; }
    if (!out_dev) { pc_set_error("pc_fill_groups: out is NULL"); return PC_ERR_ARG; }
    local.n_pairs = L;
    static const char* const fill_names[] = {"pc:fill_groups:gcs", "pc:fill_groups:jc", "pc:fill_groups:pocp", "pc:fill_groups:af", "pc:fill_groups:aai", "pc:fill_groups:peq"};
    PcGroupsHost gh;
    PcUnitDomain dom; dom.groups = &gh;
    return fill_domain(c, "pc_fill_groups", fill_names, dom, metric, ppos, as_distance, out_dev, stream, local, stats, [&]() -> int {
        // the per-position tables and the tile list
        std::vector<int32_t> h_genome(members, members + M), h_end((size_t)M), h_trow, h_tcol;
        std::vector<int64_t> h_rowbase((size_t)M + 1);
        {
            int64_t at = 0;
            for (int g = 0; g < n_groups; ++g)
                for (int64_t p = group_off[g], e = group_off[g + 1]; p < e; ++p) { h_end[p] = (int32_t)e; h_rowbase[p] = at; at += e - p - 1; }
            h_rowbase[M] = at;                                                  // = L
            std::vector<int32_t> lo, hi;
            group_block_ranges(group_off, n_groups, M, lo, hi);
            gh.nblocks = (int)lo.size();
            gh.block_tile.resize(lo.size() + 1); gh.block_slot.resize(lo.size() + 1);
            for (size_t a = 0; a < lo.size(); ++a) {
                gh.block_tile[a] = (int64_t)h_trow.size(); gh.block_slot[a] = h_rowbase[a * PC_GROUP_TILE];
                for (int32_t b = lo[a]; b <= hi[a]; ++b) { h_trow.push_back((int32_t)a); h_tcol.push_back(b); }
            }
            gh.block_tile[lo.size()] = (int64_t)h_trow.size(); gh.block_slot[lo.size()] = L;
        }
        if ((rc = upload_vec(c->b_grp_genome, h_genome)) || (rc = upload_vec(c->b_grp_end, h_end)) || (rc = upload_vec(c->b_grp_rowbase, h_rowbase)) ||
            (rc = upload_vec(c->b_grp_trow, h_trow)) || (rc = upload_vec(c->b_grp_tcol, h_tcol))) return rc;
        gh.dev = PcGroups{(int32_t)M, 0, c->b_grp_genome.as<int32_t>(), c->b_grp_end.as<int32_t>(), c->b_grp_rowbase.as<int64_t>(),
                          c->b_grp_trow.as<int32_t>(), c->b_grp_tcol.as<int32_t>(), 0};
        return PC_OK;
    });
}

extern "C" int pc_fill_groups(pc_ctx* c, int metric, int as_distance, const int32_t* members, const int64_t* group_off, int n_groups,
                              double* out_host, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_groups: upload first"); return PC_ERR_STATE; }
    const int64_t L = (n_groups > 0 && group_off) ? pc_group_pair_offsets(group_off, n_groups, nullptr) : 0;
    if (L > 0 && !out_host) { pc_set_error("pc_fill_groups: out is NULL"); return PC_ERR_ARG; }
    if (L > 0 && group_off[n_groups] > 0x7fffffffLL) { pc_set_error("pc_fill_groups: %lld members exceed 2^31-1", (long long)group_off[n_groups]); return PC_ERR_ARG; }
    return fill_to_host(c, L, out_host, true,
                        [&](void* out_dev, void* st) { return pc_fill_groups_dev(c, metric, as_distance, members, group_off, n_groups, out_dev, st, stats); });
}

// ---- pair-list fill: the pairs the caller names, METRICS[metric](genomes[src[k]], genomes[tgt[k]]) for every entry k, f64[n_pairs] in the
// caller's order.  The list is oriented (src is the reference's `source`), may repeat a pair and may hold the diagonal (src == tgt: 1 -
// as_distance).  It is sorted on the device by (target, source) with the caller's index as the value; the walker then runs over blocks of
// PC_PAIR_BLOCK sorted slots (k_walk_pairs) and scatters each value to its entry.
extern "C" int pc_pair_block(void) { return PC_PAIR_BLOCK; }

// What both forms check before anything is allocated or launched, in one pass over the list; *n_live: the entries with src != tgt.
// Returns PC_OK with *n_live = -1 when there is nothing to do (n_pairs == 0).
static int pairs_check(const pc_ctx* c, int* metric, int* ppos, const int32_t* src, const int32_t* tgt, int64_t n_pairs, const void* out, int64_t* n_live) {
    int rc = PC_OK;
    *n_live = -1;
    if ((rc = fill_check(c, "pc_fill_pairs", "a pair-list fill", metric, ppos))) return rc;
    if (n_pairs < 0) { pc_set_error("pc_fill_pairs: n_pairs %lld", (long long)n_pairs); return PC_ERR_ARG; }
    if (n_pairs == 0) return PC_OK;
    if (n_pairs > 0x7fffffffLL) { pc_set_error("pc_fill_pairs: %lld pairs exceed the 2^31-1 one call takes", (long long)n_pairs); return PC_ERR_LIMIT; }
    if (!src || !tgt || !out) { pc_set_error("pc_fill_pairs: %s is NULL", !src ? "src" : !tgt ? "tgt" : "out"); return PC_ERR_ARG; }
    const int N = c->dev.N;
    int64_t live = 0;
    for (int64_t k = 0; k < n_pairs; ++k) {
        if (src[k] < 0 || src[k] >= N || tgt[k] < 0 || tgt[k] >= N) {
            pc_set_error("pc_fill_pairs: entry %lld is (%d, %d); genome indices lie in [0, %d)", (long long)k, src[k], tgt[k], N); return PC_ERR_ARG;
        }
        live += src[k] != tgt[k];
    }
    if ((rc = fill_check_residues(c, "pc_fill_pairs", *metric))) return rc;
    *n_live = live;
    return PC_OK;
}

// the checked list (L > 0 entries, n_live of them off the diagonal) onto the device, sorted, and filled: o's one metric, or its joint set
static int fill_pairs_run(pc_ctx* c, const PcFillOut& o, int ppos, int as_distance, const int32_t* src, const int32_t* tgt, int64_t L, int64_t n_live,
                          void* stream, pc_stats* stats) {
    int rc = PC_OK;
    PC_ON_DEVICE(c);
    static const char* const fill_names[] = {"pc:fill_pairs:gcs", "pc:fill_pairs:jc", "pc:fill_pairs:pocp", "pc:fill_pairs:af", "pc:fill_pairs:aai", "pc:fill_pairs:peq"};
    const int metric = o.metric;
    PcRange range(o.mask ? "pc:fill_pairs:joint" : fill_names[metric]);
    hipStream_t st = (hipStream_t)stream;
    pc_stats local; memset(&local, 0, sizeof(local));
    local.n_pairs = n_live;
    if ((rc = wait_last_work(c, st, false))) return rc;
    int key_bits = 33;
    while (key_bits < 64 && ((int64_t)1 << (key_bits - 32)) < c->dev.N) ++key_bits;
    const size_t sort_bytes = pc_sort_temp_bytes(L, key_bits);
    if ((rc = upload_raw(c->b_pr_src, src, (size_t)L * 4)) || (rc = upload_raw(c->b_pr_tgt, tgt, (size_t)L * 4))) return rc;
    if ((rc = c->b_pr_at.ensure((size_t)L * 4)) || (rc = c->b_key0.ensure((size_t)L * 8)) || (rc = c->b_key1.ensure((size_t)L * 8)) ||
        (rc = c->b_val0.ensure((size_t)L * 4)) || (rc = c->b_sort_tmp.ensure(std::max<size_t>(sort_bytes, 16)))) return abi_rc(rc);
    PC_HIP(hipEventRecord(c->ev[0], st));
    // the sort: (target << 32 | source, entry) -> slots; the plan buffers it borrows are free until the first plan of the fill
    if ((rc = pc_launch_pair_keys(c->b_pr_src.as<int32_t>(), c->b_pr_tgt.as<int32_t>(), c->b_key0.as<unsigned long long>(), c->b_val0.as<uint32_t>(), L, st)) ||
        (rc = pc_sort_pairs(c->b_sort_tmp.p, c->b_sort_tmp.cap, c->b_key0.as<unsigned long long>(), c->b_key1.as<unsigned long long>(),
                            c->b_val0.as<uint32_t>(), c->b_pr_at.as<uint32_t>(), L, key_bits, st)) ||
        (rc = pc_launch_pair_split(c->b_key1.as<unsigned long long>(), c->b_pr_src.as<int32_t>(), c->b_pr_tgt.as<int32_t>(), L, st))) {
        (void)mark_work(c, st); return rc;
    }
    const bool split_times = stats && metric < PC_AAI;                     // a set metric: ms_plan is the sort, ms_reduce the walker alone
    if (split_times) PC_HIP(hipEventRecord(c->ev[1], st));
    PcPairsHost ph;
    ph.dev = PcPairs{L, c->b_pr_src.as<int32_t>(), c->b_pr_tgt.as<int32_t>(), c->b_pr_at.as<uint32_t>(), 0};
    ph.nblocks = (int)((L + PC_PAIR_BLOCK - 1) / PC_PAIR_BLOCK);
    PcUnitDomain dom; dom.pairs = &ph;
    rc = fill_units(c, dom, o, ppos, as_distance ? 1 : 0, st, local, stats != nullptr);
    if (rc != PC_OK && metric < PC_AAI) (void)mark_work(c, st);            // (the sort is in flight; the aligned routes are marked by the close)
    rc = fill_close(c, metric, st, rc, local, stats, false);
    if (rc == PC_OK && split_times) {                                      // (the close has waited for ev[3])
        PC_HIP(hipEventElapsedTime(&stats->ms_plan, c->ev[0], c->ev[1]));
        PC_HIP(hipEventElapsedTime(&stats->ms_reduce, c->ev[1], c->ev[3]));
    }
    return rc;
}

extern "C" int pc_fill_pairs_dev(pc_ctx* c, int metric, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                                 void* out_dev, void* stream, pc_stats* stats) {
    int ppos = 0, rc = PC_OK;
    int64_t n_live = 0;
    if ((rc = pairs_check(c, &metric, &ppos, src, tgt, n_pairs, out_dev, &n_live))) return rc;
    if (n_live < 0) { if (stats) memset(stats, 0, sizeof(*stats)); return PC_OK; }
    return fill_pairs_run(c, PcFillOut(metric, (double*)out_dev), ppos, as_distance, src, tgt, n_pairs, n_live, stream, stats);
}

extern "C" int pc_fill_pairs(pc_ctx* c, int metric, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                             double* out_host, pc_stats* stats) {
    int ppos = 0, rc = PC_OK;
    int64_t n_live = 0;
    if ((rc = pairs_check(c, &metric, &ppos, src, tgt, n_pairs, out_host, &n_live))) return rc;
    if (n_live < 0) { if (stats) memset(stats, 0, sizeof(*stats)); return PC_OK; }
    return fill_to_host(c, n_pairs, out_host, true,
                        [&](void* out_dev, void* st) { return fill_pairs_run(c, PcFillOut(metric, (double*)out_dev), ppos, as_distance, src, tgt, n_pairs, n_live, st, stats); });
}

// ---- joint fills: up to six metrics of every pair off ONE plan and ONE alignment pass.  peq = round(round(af, 6) * round(aai, 6), 6)
// computes af and aai on its way, and its walk visits every shared pham, which is all gcs, jc and pocp read: the PCW_JOINT walk
// (pc_walk.hip) is the peq fill's reduce with one store per metric asked for.  COUNT, plan, align, the chunking and the stats are the
// peq fill's own (fill_aligned / fill_units over a PcFillOut with a mask); every value is the single-metric fill's, bit for bit.

// What both domains check of a joint call before anything of their own: the context as every fill (an unsharded one), then the set
static int joint_check(const pc_ctx* c, const char* who, uint32_t metrics, void* const out[6]) {
    int metric = PC_PEQ, rc = PC_OK;
    if ((rc = fill_check(c, who, "a joint fill", &metric, nullptr))) return rc;
    if (!metrics) { pc_set_error("%s: the metric set is empty", who); return PC_ERR_ARG; }
    if (metrics & ~PC_JOINT_ALL) {
        pc_set_error("%s: metric set 0x%x has a bit above PC_PEQ (aai_ppos is another alignment pass: pc_fill)", who, metrics); return PC_ERR_ARG;
    }
    if (!(metrics & (1u << PC_AAI | 1u << PC_PEQ))) {
        pc_set_error("%s: metric set 0x%x holds neither aai nor peq; gcs / jc / pocp / af alone are four millisecond fills and share no alignment pass (pc_fill)", who, metrics);
        return PC_ERR_ARG;
    }
    if (!out) { pc_set_error("%s: out is NULL", who); return PC_ERR_ARG; }
    static const char* const names[] = {"gcs", "jc", "pocp", "af", "aai", "peq"};
    for (int m = 0; m < 6; ++m)
        if ((metrics >> m & 1u) && !out[m]) { pc_set_error("%s: out[%d] (%s) is NULL", who, m, names[m]); return PC_ERR_ARG; }
    return PC_OK;
}

// The host forms: b_out sized for the set's arrays of n doubles each, the device form run into them on the context's stream, each
// array copied to its caller's, the stream drained.  wait: as fill_to_host.
template <class Fill> static int joint_to_host(pc_ctx* c, uint32_t metrics, int64_t n, double* const host[6], bool wait, Fill fill_dev) {
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    if (wait && (rc = wait_last_work(c, c->stream, false))) return rc;
    const int64_t each = std::max<int64_t>(n, 1);
    if ((rc = c->b_out.ensure((size_t)__builtin_popcount(metrics) * each * 8))) return abi_rc(rc);
    void* dev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int k = 0;
    for (int m = 0; m < 6; ++m) if (metrics >> m & 1u) dev[m] = c->b_out.as<double>() + each * k++;
    if ((rc = fill_dev(dev, c->stream))) return rc;
    for (int m = 0; m < 6 && n > 0; ++m) if (dev[m]) PC_HIP(hipMemcpyAsync(host[m], dev[m], n * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    c->busy = false;
    return PC_OK;
}

extern "C" int pc_fill_joint_dev(pc_ctx* c, uint32_t metrics, int as_distance, void* const out_dev[6], void* stream, pc_stats* stats) {
    int rc = PC_OK;
    if ((rc = joint_check(c, "pc_fill_joint", metrics, out_dev))) return rc;
    if ((rc = fill_check_residues(c, "pc_fill_joint", PC_PEQ))) return rc;
    PC_ON_DEVICE(c);
    PcRange range("pc:fill:joint");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = wait_last_work(c, st, true))) return rc;
    pc_stats local; memset(&local, 0, sizeof(local));
    local.n_pairs = c->shard_pairs;
    PC_HIP(hipEventRecord(c->ev[0], st));
    rc = fill_aligned(c, PcFillOut(metrics, out_dev), 0, as_distance ? 1 : 0, 1, st, local, stats != nullptr);
    return fill_close(c, PC_PEQ, st, rc, local, stats, true);
}

extern "C" int pc_fill_joint(pc_ctx* c, uint32_t metrics, int as_distance, double* const out_condensed[6], pc_stats* stats) {
    int rc = PC_OK;
    if ((rc = joint_check(c, "pc_fill_joint", metrics, (void* const*)out_condensed))) return rc;
    return joint_to_host(c, metrics, (int64_t)c->dev.N * (c->dev.N - 1) / 2, out_condensed, false,
                         [&](void* const* out_dev, void* st) { return pc_fill_joint_dev(c, metrics, as_distance, out_dev, st, stats); });
}

extern "C" int pc_fill_pairs_joint_dev(pc_ctx* c, uint32_t metrics, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                                       void* const out_dev[6], void* stream, pc_stats* stats) {
    int metric = PC_PEQ, ppos = 0, rc = PC_OK;
    int64_t n_live = 0;
    if ((rc = joint_check(c, "pc_fill_pairs_joint", metrics, out_dev))) return rc;
    if ((rc = pairs_check(c, &metric, &ppos, src, tgt, n_pairs, out_dev, &n_live))) return rc;
    if (n_live < 0) { if (stats) memset(stats, 0, sizeof(*stats)); return PC_OK; }
    return fill_pairs_run(c, PcFillOut(metrics, out_dev), 0, as_distance, src, tgt, n_pairs, n_live, stream, stats);
}

extern "C" int pc_fill_pairs_joint(pc_ctx* c, uint32_t metrics, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                                   double* const out[6], pc_stats* stats) {
    int metric = PC_PEQ, ppos = 0, rc = PC_OK;
    int64_t n_live = 0;
    if ((rc = joint_check(c, "pc_fill_pairs_joint", metrics, (void* const*)out))) return rc;
    if ((rc = pairs_check(c, &metric, &ppos, src, tgt, n_pairs, out, &n_live))) return rc;
    if (n_live < 0) { if (stats) memset(stats, 0, sizeof(*stats)); return PC_OK; }
    return joint_to_host(c, metrics, n_pairs, out, true, [&](void* const* out_dev, void* st) {
        return fill_pairs_run(c, PcFillOut(metrics, out_dev), 0, as_distance, src, tgt, n_pairs, n_live, st, stats);
    });
}


extern "C" int pc_assemble_dev(pc_ctx* c, const void* gathered_dev, int world, void* out_condensed_dev, void* stream) {
    if (!c || !c->uploaded) { pc_set_error("pc_assemble_dev: upload first"); return PC_ERR_STATE; }
    if (world != c->world) { pc_set_error("pc_assemble_dev: world %d != shard world %d", world, c->world); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    if (c->balanced)
        return pc_launch_assemble_table((const double*)gathered_dev, c->shard_stride, c->dev.N, c->b_t_rank.as<int32_t>(), c->b_t_lbase.as<int64_t>(),
                                        (double*)out_condensed_dev, (hipStream_t)stream);
    return pc_launch_assemble((const double*)gathered_dev, world, c->shard_stride, c->dev.N, (double*)out_condensed_dev,
                              (hipStream_t)stream);
}
