// pc_fill.hip -- the fill entry points of libphamclust_hip.so (pc_fill, pc_fill_borrow, pc_fill_dev, pc_fill_shard_dev,
// pc_assemble_dev, pc_fill_rows, pc_fill_rows_dev, pc_fill_groups, pc_fill_groups_dev, pc_fill_edges) and the set-metric kernel selector.
#include "pc_host.h"

#ifndef PC_COL_MIN_N
#define PC_COL_MIN_N 2200        // genomes from which k_sparse_col takes over from the popcount tiles (r05 sweep: profiles/r05/experiments/sparse_col.txt)
#endif

// Which kernel fills a set metric (measured crossovers, `profiles/r03/experiments/p_sparse64_record.txt`, `r03_z_pocp_kernel_by_density.txt`;
// PC_SET_KERNEL = popc | sparse | sparse64 | sparsecol | walker forces one where it exists, applied last, for A/B runs and for the
// tests that keep every one of them honest):
//   gcs, jc          popcount tiles; a collection of many phams (long bitmap rows, few of them shared): the 64 x 64 sparse tile
//                    kernel in its counting mode
//   pocp             popcount tiles + paralog excess; from ~2,500 genomes the 64 x 64 sparse tile kernel where pairs share few
//                    enough of the phams
//   af               the 64 x 64 sparse tile kernel (the 32 x 32 one where that kernel's preconditions fail), the column kernel from ~1,400 genomes
// The popcount tiles cost ~ pairs x bitmap words W, the sparse tiles ~ pairs x (a constant + the phams a pair shares).  Measured on
// synth(5000, P), P = 300 ... 40,000, in ms: pocp 0.15 + 0.002 W against 0.207 + 0.0085 shared (sparse wins where W > 28 + 4.3 shared:
// the synthetic collection's 79 words and 2.85 shared phams yes, 300 phams -- 5 words, 34 shared -- three times no); gcs / jc
// 0.05 + 0.0014 W against 0.155 + 0.0004 W + ~0.005 shared (W > 113 + 5.4 shared: from ~7,500 phams; at 40,000: 0.43 against 0.90).
// `shared` of an average pair = sum over phams of n_p (n_p - 1) / (N (N - 1)), counted at upload.
// The 64 x 64 kernel takes "sum == 0" for "no shared pham" and sums in 32 bits: it needs every entry value >= 1 (a
// genome with an empty translation fails that for af) and genome totals below 2^31; else af falls back to the
// 32 x 32 kernel / the shared-pham walker (crossover ~3,500 genomes), pocp to the popcount tiles.
// The choice itself is pc_set_choice: a function of pc_set_inputs alone (pc_set_kernel_choice of the C-ABI); pick_set_kernel gathers
// the inputs from the context and the environment.
static int pc_set_choice(const pc_set_inputs& in) {
    int kernel = K_POPC;
    const int metric = in.metric, Wb = in.words;
    const int P64 = std::max(1, (in.two_holder + 63) / 64) * 64;       // mask entries: the phams with two holders, in 64-id words
    const int64_t area = in.n * in.nown;
    const double shared = std::max(in.avg_shared, 0.0);
    const bool counts = metric == PC_GCS || metric == PC_JC;
    const bool s64_ok = counts ? in.max_nph < (1 << 30) : metric == PC_POCP ? in.max_ngen < (1 << 16) /* two gene counts per register */ : (in.min_gene_len >= 1 && in.max_tlen < (int64_t)1 << 31);
    if (counts) kernel = (((double)Wb > 113.0 + 5.4 * shared && area >= (int64_t)3000 * 3000) ||
                          ((double)Wb > 60.0 + 5.4 * shared && area >= (int64_t)6000 * 6000)) ? K_SPARSE64 : K_POPC;   // (the sparse tiles gain on the popcount tiles as N grows: 5,056 phams, r04 with four workgroups per CU: N = 5,000 0.162 against 0.157 ms, 6,000 0.218 / 0.219, 7,000 0.258 / 0.282, 20,000 1.56 / 2.03)
    else if (metric == PC_POCP) kernel = (s64_ok && (double)Wb > 28.0 + 4.3 * shared && area >= (int64_t)2500 * 2500) ? K_SPARSE64 : K_POPC;
    else if (s64_ok) kernel = K_SPARSE64;                                  // (af; r05, ms, 32 x 32 / 64 x 64 tiles: N = 200 0.060 / 0.058, 800 0.095 / 0.061, 1,300 0.082 / 0.069 -- since r04's dense broadcast path the larger tile wins at every size)
    else kernel = area > (int64_t)3500 * 3500 ? K_WALKER : K_SPARSE32;
    // r05: the column kernel for all four (k_sparse_col: the masks over a block of targets stay in LDS for a run of source tiles, no
    // barrier per tile) -- while its masks fit 78 KB of LDS (pocp / af: beside a table of the block's entry values).  Against the popcount tiles
    // (profiles/r05/experiments/sparse_col.txt; ms, popcount / column): 5,056 phams (79 words, 2.85 shared) N = 2,000 0.035 / 0.034,
    // 3,000 0.070 / 0.046, 8,000 0.35 / 0.20, 20,000 2.03 / 0.99; 2,500 phams (40 words) N = 5,000 0.098 / 0.110; 1,200: 0.067 / 0.146
    const int sp_mode = counts ? (metric == PC_GCS ? PCW_SPARSE_GCS : PCW_SPARSE_JC) : metric == PC_POCP ? PCW_POCP : PCW_AF;
    bool col_ok = s64_ok && pc_sparse_col_lds(sp_mode, P64) > 0;
    if (col_ok && !counts)                                             // ... pocp / af: every block's entries fit its LDS value table, as 16-bit values
        col_ok = (metric == PC_POCP || in.max_ent_len < 65536) &&      // (pocp: s64_ok already holds the gene counts below 65,536)
                 in.max_block_entries <= (int64_t)pc_sparse_col_vals_cap(P64);
    // (ms, popcount tiles / 64 x 64 sparse tiles / column -- pocp: N = 2,000 0.066 / 0.082 / 0.078, 3,000 0.137 / 0.118 / 0.083, 5,000 0.304 / 0.217 / 0.156,
    // 20,000 3.89 / 2.23 / 1.45; af: 2,000 - / 0.089 / 0.078, 3,000 - / 0.121 / 0.081, 5,000 - / 0.258 / 0.150, 20,000 - / 2.41 / 1.42)
    const int64_t col_min_n = metric == PC_AF ? 1400 : PC_COL_MIN_N;        // (af, 64 x 64 tiles / column: N = 1,000 0.062 / 0.072, 1,300 0.069 / 0.073, 1,500 0.087 / 0.074, 1,800 0.088 / 0.077)
    if (col_ok && (double)Wb > 40.0 + 8.0 * shared && area >= col_min_n * col_min_n) kernel = K_SPARSE_COL;
    if (in.forced == K_SPARSE_COL && col_ok) kernel = K_SPARSE_COL;         // a forced family is taken where it exists for the metric and its guards hold
    else if (in.forced == K_POPC && metric != PC_AF) kernel = K_POPC;
    else if (in.forced == K_SPARSE32 && !counts) kernel = K_SPARSE32;
    else if (in.forced == K_SPARSE64 && s64_ok) kernel = K_SPARSE64;
    else if (in.forced == K_WALKER && !counts) kernel = K_WALKER;
    return kernel;
}
// pc_set_inputs.max_block_entries: the targets a rank owns, ascending, in blocks of 64 as k_sparse_col takes them -- the last block of a
// shard is ragged and counts like any other
extern "C" int64_t pc_set_max_block_entries(const uint32_t* entries_per_genome, const int32_t* owned, int64_t nown) {
    if (nown < 0 || (nown > 0 && (!entries_per_genome || !owned))) { pc_set_error("pc_set_max_block_entries: bad argument"); return PC_ERR_ARG; }
    int64_t most = 0;
    for (int64_t k0 = 0; k0 < nown; k0 += 64) {
        int64_t n = 0;
        for (int64_t k = k0; k < std::min(k0 + 64, nown); ++k) n += entries_per_genome[(size_t)owned[k]];
        most = std::max(most, n);
    }
    return most;
}
extern "C" int pc_set_kernel_choice(const pc_set_inputs* in) {
    if (!in || in->metric < PC_GCS || in->metric > PC_AF || in->n < 0 || in->nown < 0 || in->nown > in->n || in->words < 1 || in->two_holder < 0) {
        pc_set_error("pc_set_kernel_choice: bad argument"); return PC_ERR_ARG;
    }
    return pc_set_choice(*in);
}
extern "C" int pc_set_launch_shape(int family, int metric, int64_t n, int64_t nown, int words, int two_holder, int n_cu, int table_top,
                                   const int32_t* knobs, pc_set_shape* out) {
    if (!out || family < K_POPC || family > K_SPARSE_COL || metric < PC_GCS || metric > PC_AF || n < 0 || n > INT32_MAX || nown < 0 || nown > n ||
        words < 1 || two_holder < 0 || table_top < 0 || (metric == PC_AF && family == K_POPC) || (metric <= PC_JC && (family == K_SPARSE32 || family == K_WALKER))) {
        pc_set_error("pc_set_launch_shape: bad argument"); return PC_ERR_ARG;
    }
    const PcSetKnobs k = knobs ? PcSetKnobs{knobs[0], knobs[1], knobs[2]} : PcSetKnobs{0, 0, 0};
    pc_set_shape_of(family, metric, (int)n, (int)nown, words, std::max(1, (two_holder + 63) / 64), n_cu, table_top, k, out);
    return PC_OK;
}
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

static int fill_impl(pc_ctx* c, int metric, int as_distance, double* out, int condensed, hipStream_t st, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("fill: upload first"); return PC_ERR_STATE; }
    if (metric < PC_GCS || metric > PC_AAI_PPOS) { pc_set_error("fill: metric %d", metric); return PC_ERR_ARG; }
    const int ppos = metric == PC_AAI_PPOS;
    if (ppos) metric = PC_AAI;
    if (!out) { pc_set_error("fill: out is NULL"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    static const char* const fill_names[] = {"pc:fill:gcs", "pc:fill:jc", "pc:fill:pocp", "pc:fill:af", "pc:fill:aai", "pc:fill:peq"};
    PcRange range(fill_names[metric]);
    int rc = PC_OK;
    // st == NULL is HIP's legacy default stream, used as such: a caller whose producers / consumers run on it (PyTorch's
    // default stream has handle 0) is ordered with these launches; the library's own streams are non-blocking
    if ((rc = wait_last_work(c, st, true))) return rc;
    const PcDev& d = c->dev;
    const int64_t Lp = c->shard_pairs;
    pc_stats local; memset(&local, 0, sizeof(local));
    local.n_pairs = Lp;
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
        if (rc != PC_OK) return rc;
        PC_HIP(hipEventRecord(c->ev[3], st));
        local.n_chunks = 1;
    } else {
        rc = fill_aligned(c, metric, ppos, as_distance, out, condensed, st, local, stats != nullptr);
        if (rc != PC_OK) { (void)mark_work(c, st); return rc == PC_ERR_NOMEM_INTERNAL ? PC_ERR_HIP : rc; }
    }
    if ((rc = mark_work(c, st))) return rc;
    if (stats) {
        PC_HIP(hipEventSynchronize(c->ev[3]));
        c->busy = false;
        PC_HIP(hipEventElapsedTime(&local.ms_total, c->ev[0], c->ev[3]));
        if (metric >= PC_AAI) {
            if (local.n_chunks == 1) {
                PC_HIP(hipEventElapsedTime(&local.ms_plan, c->ev[0], c->ev[1]));
                PC_HIP(hipEventElapsedTime(&local.ms_align, c->ev[1], c->ev[2]));
                PC_HIP(hipEventElapsedTime(&local.ms_reduce, c->ev[2], c->ev[3]));
            }
        } else {
            local.ms_reduce = local.ms_total;
        }
        *stats = local;
    }
    return PC_OK;
}

extern "C" int pc_fill_dev(pc_ctx* c, int metric, int as_distance, void* out_dev, void* stream, pc_stats* stats) {
    if (c && c->uploaded && c->world != 1) { pc_set_error("pc_fill_dev: context is sharded (%d/%d); use pc_fill_shard_dev", c->rank, c->world); return PC_ERR_STATE; }
    return fill_impl(c, metric, as_distance, (double*)out_dev, 1, (hipStream_t)stream, stats);
}

extern "C" int pc_fill(pc_ctx* c, int metric, int as_distance, double* out_condensed, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill: upload first"); return PC_ERR_STATE; }
    if (!out_condensed) { pc_set_error("pc_fill: out is NULL"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    const int64_t np = (int64_t)c->dev.N * (c->dev.N - 1) / 2;
    if ((rc = c->b_out.ensure(std::max<int64_t>(np, 1) * 8))) return abi_rc(rc);
    if ((rc = pc_fill_dev(c, metric, as_distance, c->b_out.p, c->stream, stats))) return rc;
    if (np) PC_HIP(hipMemcpyAsync(out_condensed, c->b_out.p, np * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    c->busy = false;
    return PC_OK;
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
    const size_t bytes = (size_t)std::max<int64_t>(np, 1) * 8;
    if ((rc = c->b_out.ensure(bytes))) return abi_rc(rc);
    if ((rc = c->h_out.ensure(bytes))) return rc;
    if ((rc = pc_fill_dev(c, metric, as_distance, c->b_out.p, c->stream, stats))) return rc;
    if (np) PC_HIP(hipMemcpyAsync(c->h_out.p, c->b_out.p, (size_t)np * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    c->busy = false;
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

// ---- rows fill: the query genomes rows[0..n_rows) against every other genome, f64[n_rows][N].  The set metrics always run on
// the rows walker (no selector: pc_last_set_kernel / pc_last_set_launch keep reporting the last whole fill); aai / peq run
// COUNT -> plan -> align -> reduce over ranges of the rows (fill_rows_aligned).
extern "C" int pc_fill_rows_dev(pc_ctx* c, int metric, int as_distance, const int32_t* rows, int n_rows, void* out_dev, void* stream, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_rows: upload first"); return PC_ERR_STATE; }
    if (c->world != 1) { pc_set_error("pc_fill_rows: context is sharded (%d/%d); a rows fill is a one-GPU call on an unsharded context", c->rank, c->world); return PC_ERR_STATE; }
    if (metric < PC_GCS || metric > PC_AAI_PPOS) { pc_set_error("pc_fill_rows: metric %d", metric); return PC_ERR_ARG; }
    const int ppos = metric == PC_AAI_PPOS;
    if (ppos) metric = PC_AAI;
    if (n_rows < 0) { pc_set_error("pc_fill_rows: n_rows %d", n_rows); return PC_ERR_ARG; }
    pc_stats local; memset(&local, 0, sizeof(local));
    if (n_rows == 0) { if (stats) *stats = local; return PC_OK; }
    if (!rows || !out_dev) { pc_set_error("pc_fill_rows: %s is NULL", rows ? "out" : "rows"); return PC_ERR_ARG; }
    const PcDev& d = c->dev;
    const int N = d.N;
    for (int k = 0; k < n_rows; ++k)
        if (rows[k] < 0 || rows[k] >= N || (k > 0 && rows[k] <= rows[k - 1])) {
            pc_set_error("pc_fill_rows: rows must be strictly ascending genome indices below %d (rows[%d] = %d)", N, k, rows[k]); return PC_ERR_ARG;
        }
    if (metric >= PC_AAI && !c->residues_ready) { pc_set_error("pc_fill_rows: aai / peq need the residues on the device (pc_upload, or pc_upload_residues after pc_upload_sets)"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    static const char* const fill_names[] = {"pc:fill_rows:gcs", "pc:fill_rows:jc", "pc:fill_rows:pocp", "pc:fill_rows:af", "pc:fill_rows:aai", "pc:fill_rows:peq"};
    PcRange range(fill_names[metric]);
    hipStream_t st = (hipStream_t)stream;
    int rc = PC_OK;
    if ((rc = wait_last_work(c, st, false))) return rc;                    // (the domain tables below are rewritten by a blocking copy: nothing may still read them)
    std::vector<int32_t> h_rows(rows, rows + n_rows), h_row_of((size_t)N, -1);
    for (int k = 0; k < n_rows; ++k) h_row_of[rows[k]] = k;
    if ((rc = upload_vec(c->b_rows, h_rows)) || (rc = upload_vec(c->b_row_of, h_row_of))) return rc;
    const PcRows rw{n_rows, c->b_rows.as<int32_t>(), c->b_row_of.as<int32_t>()};
    local.n_pairs = (int64_t)n_rows * (N - 1) - (int64_t)n_rows * (n_rows - 1) / 2;
    as_distance = as_distance ? 1 : 0;
    PC_HIP(hipEventRecord(c->ev[0], st));
    if (metric < PC_AAI) {
        PcWalkArgs a; memset(&a, 0, sizeof(a));
        a.out = (double*)out_dev; a.as_distance = as_distance;
        const int mode = metric == PC_GCS ? PCW_GCS : metric == PC_JC ? PCW_JC : metric == PC_POCP ? PCW_POCP : PCW_AF;
        if ((rc = pc_launch_walk_rows(mode, d, rw, 0, n_rows, a, st))) return rc;
        PC_HIP(hipEventRecord(c->ev[3], st));
        local.n_chunks = 1;
    } else {
        rc = fill_rows_aligned(c, rw, metric, ppos, as_distance, (double*)out_dev, st, local, stats != nullptr);
        if (rc != PC_OK) { (void)mark_work(c, st); return abi_rc(rc); }
    }
    if ((rc = mark_work(c, st))) return rc;
    if (stats) {
        PC_HIP(hipEventSynchronize(c->ev[3]));
        c->busy = false;
        PC_HIP(hipEventElapsedTime(&local.ms_total, c->ev[0], c->ev[3]));
        if (metric < PC_AAI) local.ms_reduce = local.ms_total;
        *stats = local;
    }
    return PC_OK;
}

extern "C" int pc_fill_rows(pc_ctx* c, int metric, int as_distance, const int32_t* rows, int n_rows, double* out_host, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_rows: upload first"); return PC_ERR_STATE; }
    if (n_rows > 0 && !out_host) { pc_set_error("pc_fill_rows: out is NULL"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    const int64_t cells = (int64_t)std::max(n_rows, 0) * c->dev.N;
    if ((rc = wait_last_work(c, c->stream, false))) return rc;             // (b_out may still be read by a fill left on another stream)
    if ((rc = c->b_out.ensure(std::max<int64_t>(cells, 1) * 8))) return abi_rc(rc);
    if ((rc = pc_fill_rows_dev(c, metric, as_distance, rows, n_rows, c->b_out.p, c->stream, stats))) return rc;
    if (n_rows > 0 && cells) PC_HIP(hipMemcpyAsync(out_host, c->b_out.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    c->busy = false;
    return PC_OK;
}

// ---- groups fill: every pair (s, t), s < t, of two genomes in the same group of a caller-given family of groups, as the groups'
// condensed triangles end to end, f64[L].  members[M]: genome indices group by group, strictly ascending inside a group (position
// order = index order, so every pair keeps the whole fill's orientation); group_off[G+1]: each group's range.  Groups may share
// genomes; a group of 0 or 1 members has no pair.  The set metrics always run on the groups walker (no selector: pc_last_set_kernel /
// pc_last_set_launch keep reporting the last whole fill); aai / peq run COUNT -> plan -> align -> reduce over ranges of row blocks
// (fill_groups_aligned).

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
    if (!c || !c->uploaded) { pc_set_error("pc_fill_groups: upload first"); return PC_ERR_STATE; }
    if (c->world != 1) { pc_set_error("pc_fill_groups: context is sharded (%d/%d); a groups fill is a one-GPU call on an unsharded context", c->rank, c->world); return PC_ERR_STATE; }
    if (metric < PC_GCS || metric > PC_AAI_PPOS) { pc_set_error("pc_fill_groups: metric %d", metric); return PC_ERR_ARG; }
    const int ppos = metric == PC_AAI_PPOS;
    if (ppos) metric = PC_AAI;
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
    const PcDev& d = c->dev;
    const int N = d.N;
    for (int g = 0; g < n_groups; ++g)
        for (int64_t p = group_off[g]; p < group_off[g + 1]; ++p)
            if (members[p] < 0 || members[p] >= N || (p > group_off[g] && members[p] <= members[p - 1])) {
                pc_set_error("pc_fill_groups: a group's members must be strictly ascending genome indices below %d (group %d, members[%lld] = %d)",
                             N, g, (long long)p, members[p]);
                return PC_ERR_ARG;
            }
    if (L == 0) { if (stats) *stats = local; return PC_OK; }
    if (!out_dev) { pc_set_error("pc_fill_groups: out is NULL"); return PC_ERR_ARG; }
    if (metric >= PC_AAI && !c->residues_ready) { pc_set_error("pc_fill_groups: aai / peq need the residues on the device (pc_upload, or pc_upload_residues after pc_upload_sets)"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    static const char* const fill_names[] = {"pc:fill_groups:gcs", "pc:fill_groups:jc", "pc:fill_groups:pocp", "pc:fill_groups:af", "pc:fill_groups:aai", "pc:fill_groups:peq"};
    PcRange range(fill_names[metric]);
    hipStream_t st = (hipStream_t)stream;
    int rc = PC_OK;
    if ((rc = wait_last_work(c, st, false))) return rc;                    // (the domain tables below are rewritten by a blocking copy: nothing may still read them)
    // the per-position tables and the tile list
    PcGroupsHost gh;
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
    local.n_pairs = L;
    as_distance = as_distance ? 1 : 0;
    PC_HIP(hipEventRecord(c->ev[0], st));
    if (metric < PC_AAI) {
        PcWalkArgs a; memset(&a, 0, sizeof(a));
        a.out = (double*)out_dev; a.as_distance = as_distance;
        const int mode = metric == PC_GCS ? PCW_GCS : metric == PC_JC ? PCW_JC : metric == PC_POCP ? PCW_POCP : PCW_AF;
        if ((rc = pc_launch_walk_groups(mode, d, gh.dev, 0, (int64_t)h_trow.size(), a, st))) return rc;
        PC_HIP(hipEventRecord(c->ev[3], st));
        local.n_chunks = 1;
    } else {
        rc = fill_groups_aligned(c, gh, metric, ppos, as_distance, (double*)out_dev, st, local, stats != nullptr);
        if (rc != PC_OK) { (void)mark_work(c, st); return abi_rc(rc); }
    }
    if ((rc = mark_work(c, st))) return rc;
    if (stats) {
        PC_HIP(hipEventSynchronize(c->ev[3]));
        c->busy = false;
        PC_HIP(hipEventElapsedTime(&local.ms_total, c->ev[0], c->ev[3]));
        if (metric < PC_AAI) local.ms_reduce = local.ms_total;
        *stats = local;
    }
    return PC_OK;
}

extern "C" int pc_fill_groups(pc_ctx* c, int metric, int as_distance, const int32_t* members, const int64_t* group_off, int n_groups,
                              double* out_host, pc_stats* stats) {
    if (!c || !c->uploaded) { pc_set_error("pc_fill_groups: upload first"); return PC_ERR_STATE; }
    const int64_t L = (n_groups > 0 && group_off) ? pc_group_pair_offsets(group_off, n_groups, nullptr) : 0;
    if (L > 0 && !out_host) { pc_set_error("pc_fill_groups: out is NULL"); return PC_ERR_ARG; }
    if (L > 0 && group_off[n_groups] > 0x7fffffffLL) { pc_set_error("pc_fill_groups: %lld members exceed 2^31-1", (long long)group_off[n_groups]); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    int rc = PC_OK;
    if ((rc = wait_last_work(c, c->stream, false))) return rc;             // (b_out may still be read by a fill left on another stream)
    if ((rc = c->b_out.ensure(std::max<int64_t>(L, 1) * 8))) return abi_rc(rc);
    if ((rc = pc_fill_groups_dev(c, metric, as_distance, members, group_off, n_groups, c->b_out.p, c->stream, stats))) return rc;
    if (L > 0) PC_HIP(hipMemcpyAsync(out_host, c->b_out.p, L * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    c->busy = false;
    return PC_OK;
}

// ---- edge-list fill: the pairs whose value passes a threshold, as (source, target, value) arrays sorted by target, then source --
// what matrix_to_adjacency(skip_zero) writes and SymMatrix.nearest_neighbors answers from the dense matrix (matrix.py:536-551,
// 265-296), without the dense matrix ever crossing PCIe.  The call walks successive contiguous ranges of target genomes ("slabs":
// pc_chunk_plan over count[t] = t under slab_bytes / 8 pairs, at most 2^31-1 so that u32 counts and offsets do); each range is
// installed as a PcShard (owned = t0 .. t1-1, shard-local layout), filled by fill_impl into the context's slab buffer, compacted
// (count -> scan -> one 4-byte read-back -> emit, pc_edges.hip) and its edges appended to the pinned host result.  Slabs in
// ascending target order make the concatenation globally ordered.  One slab is resident at a time.
#define PC_EDGE_MAX_PAIRS 0x7fffffffLL

// the caller's unsharded state, put back however the call ends (the slab shards live in buffers of their own: b_owned / b_lbase,
// the deal tables, rank / world and the stride are never touched)
namespace {
struct EdgeShardScope {
    pc_ctx* c; PcShard shard; int64_t pairs; std::vector<int32_t> owned; std::vector<int64_t> lbase;
    explicit EdgeShardScope(pc_ctx* ctx) : c(ctx), shard(ctx->shard), pairs(ctx->shard_pairs), owned(ctx->h_owned), lbase(ctx->h_lbase) {}
    ~EdgeShardScope() { c->shard = shard; c->shard_pairs = pairs; c->h_owned.swap(owned); c->h_lbase.swap(lbase); c->plan.valid = false; }
    EdgeShardScope(const EdgeShardScope&) = delete; EdgeShardScope& operator=(const EdgeShardScope&) = delete;
};
}  // namespace

extern "C" int pc_fill_edges(pc_ctx* c, int metric, int as_distance, double threshold, int64_t slab_bytes,
                             const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    if (src) *src = nullptr;
    if (tgt) *tgt = nullptr;
    if (val) *val = nullptr;
    if (n_edges) *n_edges = 0;
    if (n_slabs) *n_slabs = 0;
    if (!c || !c->uploaded) { pc_set_error("pc_fill_edges: upload first"); return PC_ERR_STATE; }
    if (!src || !tgt || !val || !n_edges || !n_slabs) { pc_set_error("pc_fill_edges: an output pointer is NULL"); return PC_ERR_ARG; }
    if (metric < PC_GCS || metric > PC_AAI_PPOS) { pc_set_error("pc_fill_edges: metric %d", metric); return PC_ERR_ARG; }
    if (threshold != threshold) { pc_set_error("pc_fill_edges: the threshold is NaN"); return PC_ERR_ARG; }
    if (slab_bytes < 0) { pc_set_error("pc_fill_edges: slab_bytes %lld", (long long)slab_bytes); return PC_ERR_ARG; }
    if (c->world != 1) { pc_set_error("pc_fill_edges: context is sharded (%d/%d); an edge-list fill is a one-GPU call on an unsharded context", c->rank, c->world); return PC_ERR_STATE; }
    if (metric >= PC_AAI && !c->residues_ready) { pc_set_error("pc_fill_edges: aai / peq need the residues on the device (pc_upload, or pc_upload_residues after pc_upload_sets)"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    PcRange range("pc:fill_edges");
    int rc = PC_OK;
    hipStream_t st = c->stream;
    const int N = c->dev.N;
    pc_stats sum; memset(&sum, 0, sizeof(sum));
    c->last_edge_ms[0] = c->last_edge_ms[1] = 0.f;
    as_distance = as_distance ? 1 : 0;
    if ((rc = wait_last_work(c, st, false))) return rc;                     // (the loan of an earlier call ends here: its buffers are rewritten)
    if ((rc = c->h_edge_src.ensure(16)) || (rc = c->h_edge_tgt.ensure(16)) || (rc = c->h_edge_val.ensure(16))) return rc;
    if (N <= 1) {
        *src = c->h_edge_src.as<int32_t>(); *tgt = c->h_edge_tgt.as<int32_t>(); *val = c->h_edge_val.as<double>();
        if (stats) *stats = sum;
        return PC_OK;
    }
    // ---- the cut: ranges of targets whose pairs fit the slab
    const int64_t np = (int64_t)N * (N - 1) / 2;
    int64_t max_pairs;
    if (slab_bytes > 0) max_pairs = std::max<int64_t>(slab_bytes / 8, 1);
    else {                                                                  // the dense triangle, or a quarter of what is free now (an aai / peq slab's plan takes its own half)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
        max_pairs = std::min<int64_t>(np, std::max<int64_t>((int64_t)((free_b + c->b_edge_slab.cap) / 4 / 8), 1));
    }
    max_pairs = std::min<int64_t>(max_pairs, PC_EDGE_MAX_PAIRS);
    std::vector<uint64_t> per_target((size_t)N);
    for (int t = 0; t < N; ++t) per_target[t] = (uint64_t)t;
    const int nsl = pc_chunk_plan(per_target.data(), N, (uint64_t)max_pairs, nullptr, 0);
    if (nsl < 0) return nsl;
    std::vector<int32_t> cut((size_t)nsl + 1);
    if ((rc = pc_chunk_plan(per_target.data(), N, (uint64_t)max_pairs, cut.data(), nsl + 1)) < 0) return rc;
    auto pairs_below = [](int64_t t) { return t * (t - 1) / 2; };           // pairs (s, t'), s < t' < t
    int64_t most = 1;
    for (int i = 0; i < nsl; ++i) most = std::max(most, pairs_below(cut[i + 1]) - pairs_below(cut[i]));
    if ((rc = c->b_edge_slab.ensure((size_t)most * 8))) return abi_rc(rc);
    if (stats) for (hipEvent_t& e : c->ev_edge) if (!e) PC_HIP(hipEventCreate(&e));
    double* const slab = c->b_edge_slab.as<double>();
    uint32_t* const h_total = c->h_plan.as<uint32_t>();

    EdgeShardScope restore(c);
    int64_t E = 0;
    std::vector<int32_t> owned; std::vector<int64_t> lbase;
    for (int i = 0; i < nsl; ++i) {
        const int t0 = cut[i], t1 = cut[i + 1];
        const int64_t Lp = pairs_below(t1) - pairs_below(t0);
        if (Lp == 0) continue;                                              // (target 0 alone: no pair)
        owned.resize((size_t)(t1 - t0)); lbase.resize((size_t)(t1 - t0) + 1);
        for (int t = t0; t < t1; ++t) { owned[t - t0] = t; lbase[t - t0] = pairs_below(t) - pairs_below(t0); }
        lbase[t1 - t0] = Lp;
        if ((rc = upload_vec(c->b_edge_owned, owned)) || (rc = upload_vec(c->b_edge_lbase, lbase))) return rc;
        // install the slab's shard as apply_shard installs one: a plan belongs to the shard it was made for, and pick_set_kernel
        // gathers its per-shard inputs (nown, max_block_entries) from what is in force
        c->plan.valid = false;
        c->shard.nown = t1 - t0; c->shard.ident = 0;
        c->shard.owned = c->b_edge_owned.as<int32_t>(); c->shard.lbase = c->b_edge_lbase.as<int64_t>();
        c->h_owned = owned; c->h_lbase = lbase; c->shard_pairs = Lp;
        pc_stats one; memset(&one, 0, sizeof(one));
        if ((rc = fill_impl(c, metric, as_distance, slab, 0, st, stats ? &one : nullptr))) return rc;
        sum.n_pairs += Lp; sum.n_alignments += one.n_alignments; sum.n_cells += one.n_cells; sum.n_tasks += one.n_tasks;
        sum.n_residue_bytes += one.n_residue_bytes; sum.n_align_launches += one.n_align_launches; sum.n_chunks += one.n_chunks;
        sum.ms_total += one.ms_total; sum.ms_plan += one.ms_plan; sum.ms_align += one.ms_align; sum.ms_reduce += one.ms_reduce;
        sum.n_distinct_alignments += one.n_distinct_alignments; sum.n_distinct_cells += one.n_distinct_cells;
        // ---- compact: count -> scan (n + 1 elements: the total falls out) -> read the total back -> emit
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
            continue;
        }
        if ((rc = c->b_edge_src.ensure((size_t)Es * 4)) || (rc = c->b_edge_tgt.ensure((size_t)Es * 4)) || (rc = c->b_edge_val.ensure((size_t)Es * 8))) return abi_rc(rc);
        if ((rc = c->h_edge_src.grow_keep((size_t)(E + Es) * 4, (size_t)E * 4)) || (rc = c->h_edge_tgt.grow_keep((size_t)(E + Es) * 4, (size_t)E * 4)) ||
            (rc = c->h_edge_val.grow_keep((size_t)(E + Es) * 8, (size_t)E * 8))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_edge[2], st));
        if ((rc = pc_launch_edge_emit(slab, Lp, as_distance, threshold, c->shard, off, c->b_edge_src.as<int32_t>(), c->b_edge_tgt.as<int32_t>(),
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
    }
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    *src = c->h_edge_src.as<int32_t>(); *tgt = c->h_edge_tgt.as<int32_t>(); *val = c->h_edge_val.as<double>();
    *n_edges = E; *n_slabs = nsl;
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
// reference's single-linkage clusters at that eps (clustering.py:4-51) -- as labels[N], the smallest member's index.  pc_fill_edges'
// walk (the same cut, the same shard install, the same restore; the loop is written out a second time so that pc_fill_edges stays
// as it is), but each filled slab goes through ONE pass, k_cc_union (pc_components.hip), over a parent[N] array that stays on the
// device from the first slab to the last; nothing is read back per slab.  After the last slab: k_cc_labels, then one D2H of
// labels[N] and the 8-byte count of passing pairs behind them.
extern "C" int pc_fill_components(pc_ctx* c, int metric, int as_distance, double threshold, int strict, int64_t slab_bytes,
                                  const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats) {
    if (labels) *labels = nullptr;
    if (n_components) *n_components = 0;
    if (n_edges) *n_edges = 0;
    if (n_slabs) *n_slabs = 0;
    if (!c || !c->uploaded) { pc_set_error("pc_fill_components: upload first"); return PC_ERR_STATE; }
    if (!labels || !n_components || !n_edges || !n_slabs) { pc_set_error("pc_fill_components: an output pointer is NULL"); return PC_ERR_ARG; }
    if (metric < PC_GCS || metric > PC_AAI_PPOS) { pc_set_error("pc_fill_components: metric %d", metric); return PC_ERR_ARG; }
    if (threshold != threshold) { pc_set_error("pc_fill_components: the threshold is NaN"); return PC_ERR_ARG; }
    if (slab_bytes < 0) { pc_set_error("pc_fill_components: slab_bytes %lld", (long long)slab_bytes); return PC_ERR_ARG; }
    if (c->world != 1) { pc_set_error("pc_fill_components: context is sharded (%d/%d); a components fill is a one-GPU call on an unsharded context", c->rank, c->world); return PC_ERR_STATE; }
    if (metric >= PC_AAI && !c->residues_ready) { pc_set_error("pc_fill_components: aai / peq need the residues on the device (pc_upload, or pc_upload_residues after pc_upload_sets)"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    PcRange range("pc:fill_components");
    int rc = PC_OK;
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
    // ---- the cut: pc_fill_edges' (ranges of targets whose pairs fit the slab)
    const int64_t np = (int64_t)N * (N - 1) / 2;
    int64_t max_pairs;
    if (slab_bytes > 0) max_pairs = std::max<int64_t>(slab_bytes / 8, 1);
    else {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = (size_t)16 << 30; }
        max_pairs = std::min<int64_t>(np, std::max<int64_t>((int64_t)((free_b + c->b_edge_slab.cap) / 4 / 8), 1));
    }
    max_pairs = std::min<int64_t>(max_pairs, PC_EDGE_MAX_PAIRS);
    std::vector<uint64_t> per_target((size_t)N);
    for (int t = 0; t < N; ++t) per_target[t] = (uint64_t)t;
    const int nsl = pc_chunk_plan(per_target.data(), N, (uint64_t)max_pairs, nullptr, 0);
    if (nsl < 0) return nsl;
    std::vector<int32_t> cut((size_t)nsl + 1);
    if ((rc = pc_chunk_plan(per_target.data(), N, (uint64_t)max_pairs, cut.data(), nsl + 1)) < 0) return rc;
    auto pairs_below = [](int64_t t) { return t * (t - 1) / 2; };           // pairs (s, t'), s < t' < t
    int64_t most = 1;
    for (int i = 0; i < nsl; ++i) most = std::max(most, pairs_below(cut[i + 1]) - pairs_below(cut[i]));
    if ((rc = c->b_edge_slab.ensure((size_t)most * 8)) || (rc = c->b_cc_parent.ensure((size_t)N * 4)) || (rc = c->b_cc_labels.ensure(label_bytes + 8))) return abi_rc(rc);
    if (stats) for (hipEvent_t& e : c->ev_cc) if (!e) PC_HIP(hipEventCreate(&e));
    double* const slab = c->b_edge_slab.as<double>();
    int32_t* const parent = c->b_cc_parent.as<int32_t>();
    unsigned long long* const d_pass = (unsigned long long*)((char*)c->b_cc_labels.p + label_bytes);
    if ((rc = pc_launch_cc_init(parent, N, d_pass, st))) return rc;

    EdgeShardScope restore(c);
    std::vector<int32_t> owned; std::vector<int64_t> lbase;
    bool pending = false;                                                   // a union pass is in flight (and, with stats, its two events recorded)
    for (int i = 0; i < nsl; ++i) {
        const int t0 = cut[i], t1 = cut[i + 1];
        const int64_t Lp = pairs_below(t1) - pairs_below(t0);
        if (Lp == 0) continue;                                              // (target 0 alone: no pair)
        owned.resize((size_t)(t1 - t0)); lbase.resize((size_t)(t1 - t0) + 1);
        for (int t = t0; t < t1; ++t) { owned[t - t0] = t; lbase[t - t0] = pairs_below(t) - pairs_below(t0); }
        lbase[t1 - t0] = Lp;
        // (a blocking copy into tables the previous slab's union pass may still read: wait for it)
        if (pending) {
            PC_HIP(hipStreamSynchronize(st));
            c->busy = false;
            if (stats) { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, c->ev_cc[0], c->ev_cc[1])); c->last_cc_ms[0] += x; }
        }
        if ((rc = upload_vec(c->b_edge_owned, owned)) || (rc = upload_vec(c->b_edge_lbase, lbase))) return rc;
        c->plan.valid = false;
        c->shard.nown = t1 - t0; c->shard.ident = 0;
        c->shard.owned = c->b_edge_owned.as<int32_t>(); c->shard.lbase = c->b_edge_lbase.as<int64_t>();
        c->h_owned = owned; c->h_lbase = lbase; c->shard_pairs = Lp;
        pc_stats one; memset(&one, 0, sizeof(one));
        if ((rc = fill_impl(c, metric, as_distance, slab, 0, st, stats ? &one : nullptr))) return rc;
        sum.n_pairs += Lp; sum.n_alignments += one.n_alignments; sum.n_cells += one.n_cells; sum.n_tasks += one.n_tasks;
        sum.n_residue_bytes += one.n_residue_bytes; sum.n_align_launches += one.n_align_launches; sum.n_chunks += one.n_chunks;
        sum.ms_total += one.ms_total; sum.ms_plan += one.ms_plan; sum.ms_align += one.ms_align; sum.ms_reduce += one.ms_reduce;
        sum.n_distinct_alignments += one.n_distinct_alignments; sum.n_distinct_cells += one.n_distinct_cells;
        if (stats) PC_HIP(hipEventRecord(c->ev_cc[0], st));
        if ((rc = pc_launch_cc_union(slab, Lp, as_distance, strict, threshold, c->shard, parent, d_pass, st))) return rc;
        if (stats) PC_HIP(hipEventRecord(c->ev_cc[1], st));
        pending = true;
    }
    if (stats) PC_HIP(hipEventRecord(c->ev_cc[2], st));
    if ((rc = pc_launch_cc_labels(parent, c->b_cc_labels.as<int32_t>(), N, st))) return rc;
    if (stats) PC_HIP(hipEventRecord(c->ev_cc[3], st));
    PC_HIP(hipMemcpyAsync(h_labels, c->b_cc_labels.p, label_bytes + 8, hipMemcpyDeviceToHost, st));
    PC_HIP(hipStreamSynchronize(st));
    c->busy = false;
    if (stats) {
        if (pending) { float x = 0.f; PC_HIP(hipEventElapsedTime(&x, c->ev_cc[0], c->ev_cc[1])); c->last_cc_ms[0] += x; }   // (the last slab's pass)
        PC_HIP(hipEventElapsedTime(&c->last_cc_ms[1], c->ev_cc[2], c->ev_cc[3]));
    }
    int32_t comps = 0;
    for (int g = 0; g < N; ++g) comps += h_labels[g] == g;
    unsigned long long passed = 0;
    memcpy(&passed, (const char*)h_labels + label_bytes, 8);
    *labels = h_labels; *n_components = comps; *n_edges = (int64_t)passed; *n_slabs = nsl;
    if (stats) *stats = sum;
    return PC_OK;
}

extern "C" int pc_last_component_times(const pc_ctx* c, float* ms_union, float* ms_labels) {
    if (!c) { pc_set_error("pc_last_component_times: NULL context"); return PC_ERR_ARG; }
    if (ms_union) *ms_union = c->last_cc_ms[0];
    if (ms_labels) *ms_labels = c->last_cc_ms[1];
    return PC_OK;
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
