// pc_set_shape.hip -- the set metrics' host arithmetic: the launch shapes of the five kernel families (pc_set_launch_shape of the C-ABI;
// every launcher takes its numbers from pc_set_shape_of) and the selector that picks the family (pc_set_choice; pc_set_kernel_choice and
// pc_set_max_block_entries of the C-ABI).  Host only, no device code, no context; the constants come from pc_pairs.h, the column kernel's
// LDS budget from pc_sparse_col.hip.  Restates nothing of metrics.py.
#include "pc_pairs.h"
#include <algorithm>
#include <stdlib.h>

PcSetKnobs pc_set_knobs_env() {
    PcSetKnobs k{0, 0, 0};
    if (const char* v = getenv("PC_POPC_TILE")) k.popc_tile = atoi(v);                  // tuning / test knob: 32 / 64
    if (const char* v = getenv("PC_S64_CHUNKS")) k.s64_chunks = atoi(v);                // test knob: at least this many chunks, so that small collections reach the one-batch instances and the forced split
    if (const char* v = getenv("PC_COL_SEG")) k.col_seg = atoi(v);
    return k;
}
bool pc_set_table_dims(int metric, int top, int* sh_dim, int* tot_dim) {
    *sh_dim = metric == PC_POCP ? 2 * top + 1 : top + 1; *tot_dim = 2 * top + 1;
    return (int64_t)*sh_dim * *tot_dim <= (4 << 20);
}
void pc_set_shape_of(int family, int metric, int N, int nown, int Wb, int sp_W, int n_cu, int table_top, const PcSetKnobs& knobs, pc_set_shape* out) {
    *out = pc_set_shape{};
    out->family = family;
    if (nown <= 0 || N <= 1) return;                                                    // (nothing is launched)
    const int mode = metric == PC_GCS ? S6_GCS : metric == PC_JC ? S6_JC : metric == PC_POCP ? PCW_POCP : PCW_AF;
    const int cu = n_cu > 0 ? n_cu : 256;
    const int P64 = sp_W * 64;                                                          // phams with at least two holders
    out->units_per_wg = 1;
    if (family == K_POPC) {
        const int64_t tiles64 = (int64_t)((N + 63) / 64) * ((nown + 63) / 64);
        const bool small = knobs.popc_tile ? knobs.popc_tile == 32 : tiles64 / 2 < PC_SMALL_GRID_TILES;     // about half of the tiles are live
        out->tile = small ? 32 : 64;
        const int ntx = (N + out->tile - 1) / out->tile, nty = (nown + out->tile - 1) / out->tile;
        out->super_edge = (int)pc_super_edge((unsigned)ntx, (unsigned)nty);
        out->grid = out->units = (int)pc_tile_grid(ntx, nty);
        int sh_dim, tot_dim;
        out->table = pc_set_table_dims(metric, table_top, &sh_dim, &tot_dim) ? 1 : 0;
    } else if (family == K_SPARSE32 || family == K_WALKER) {
        out->tile = TS;
        const int ntx = (N + TS - 1) / TS, nty = (nown + TS - 1) / TS;
        out->super_edge = (int)pc_super_edge((unsigned)ntx, (unsigned)nty);
        out->grid = out->units = (int)pc_tile_grid(ntx, nty);
        if (family == K_SPARSE32) {
            // colmask chunk: all phams at once while that leaves three workgroups per CU (48 KB each), else 8,192 at a time
            const int V64 = Wb * 64;
            out->chunk = V64 <= 10240 ? V64 : 8192;
            out->chunks = (V64 + out->chunk - 1) / out->chunk;
            out->lds = (int)((size_t)out->chunk * 4 + (size_t)SP_T * SP_T * 8);
        }
    } else if (family == K_SPARSE64) {
        // mask chunk: all phams at once while two workgroups still fit a CU (8 B per pham + 17 KB of accumulators: 7,680 phams), else the
        // fewest equal chunks of at most that many
        // ... except that 2,048 ... 7,680 phams are split in two from ~4,000 genomes: the one-batch instances need 59 (gcs / jc), 78 (af) and --
        // held there by the launch bound, 4 dwords of scratch -- 80 (pocp) registers, and with 20 KB of masks three workgroups fit a CU instead
        // of two (N = 20,000, 5,056 phams: jc 2.06 -> 1.79 ms, af 2.89 -> 2.60, pocp 2.61 -> 2.42; below: af at N = 3,000 0.150 ms whole, 0.165 split)
        const int chunk_cap = pc_s6_dense(mode, 2) ? 6912 : 7680;                       // (6 KB of broadcast staging beside the accumulators)
        int n_chunks = (P64 + chunk_cap - 1) / chunk_cap;
        if (n_chunks == 1 && P64 >= 2048 && (int64_t)N * nown >= (int64_t)4000 * 4000) n_chunks = 2;
        if (knobs.s64_chunks > n_chunks && knobs.s64_chunks <= P64 / 64) n_chunks = knobs.s64_chunks;
        const int CH = (P64 / 64 + n_chunks - 1) / n_chunks * 64;                       // equal chunks (synth(20000,20000): 5 x 4,096: jc 2.67 ms, 3 x 6,720: 2.5)
        out->tile = S6_T;
        out->chunk = CH; out->chunks = (P64 + CH - 1) / CH;
        out->batches = CH < P64 ? 1 : 2;
        out->dense = pc_s6_dense(mode, out->batches) ? 1 : 0;
        out->lds = (int)((size_t)CH * 8 + (size_t)S6_T * S6_LD * 4 + (out->dense ? (size_t)S6_WAVES * S6_STAGE_DWORDS * 4 : 0));
        const int ntx = (N + S6_T - 1) / S6_T, nty = (nown + S6_T - 1) / S6_T;
        out->super_edge = (int)pc_super_edge((unsigned)ntx, (unsigned)nty, S6_SUPER);
        const unsigned n_units = pc_tile_grid(ntx, nty, S6_SUPER);
        const unsigned resident = (unsigned)(2 * cu + 7) / 8u * 8u;                     // (the context's own device: pc_ctx_create asked it)
        // three units per workgroup (see the kernel); small matrices: one unit each, up to four times the workgroups that fit the chip
        // at once (N = 2,000: 0.158 ms with two units per workgroup, 0.129 with one)
        const unsigned want = std::max(std::min(n_units, 4u * resident), ((n_units + 2u) / 3u + 7u) / 8u * 8u);
        const unsigned grid = std::min(n_units, want);
        out->units = (int)n_units; out->grid = (int)grid;
        out->units_per_wg = (int)((n_units + grid - 1) / grid);
    } else {                                                                            // K_SPARSE_COL
        out->tile = S6_T;
        out->vals_cap = metric == PC_POCP || metric == PC_AF ? pc_sparse_col_vals_cap(P64) : 0;
        out->lds = (int)pc_sparse_col_lds(mode, P64);                                   // 0: the masks do not fit, the launcher refuses
        out->chunk = P64; out->chunks = 1;
        const int nty = (nown + S6_T - 1) / S6_T, ntx = (N + S6_T - 1) / S6_T;
        // source tiles per unit: as many as leave ~2 units per workgroup slot of the chip (2 slots per CU), at most S7_SEG.  Measured, jc, ms
        // (profiles/r05/experiments/sparse_col.txt): N = 2,000 / 3,000 / 5,000 / 20,000 with 1 tile per unit 0.034 / 0.046 / 0.105 / 1.27,
        // 2: 0.047 / 0.049 / 0.092 / 1.10, 4: 0.058 / 0.060 / 0.093 / 1.02, 8: 0.081 / 0.083 / 0.100 / 0.99, 16: 0.126 / 0.127 / 0.166 / 1.005
        const int64_t live_tiles = (int64_t)nty * ntx / 2 + nty;
        int seg = (int)std::max<int64_t>(1, std::min<int64_t>(S7_SEG, live_tiles / (4 * (int64_t)cu)));
        if (knobs.col_seg >= 1 && knobs.col_seg <= 64) seg = knobs.col_seg;
        out->seg = seg; out->runs = (ntx + seg - 1) / seg;
        out->grid = out->units = (int)(((unsigned)nty + 7u) / 8u * 8u * ((unsigned)out->runs + 2u));     // (runs 0, 1: every block's diagonal run and the one below; then the runs, highest first)
    }
}

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
// The choice itself is pc_set_choice: a function of pc_set_inputs alone (pc_set_kernel_choice of the C-ABI); pick_set_kernel
// (pc_fill.hip) gathers the inputs from the context and the environment.
int pc_set_choice(const pc_set_inputs& in) {
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
