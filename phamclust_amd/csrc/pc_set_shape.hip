// pc_set_shape.hip -- the launch shapes of the five set-metric families as host arithmetic (pc_set_launch_shape of the C-ABI): every
// launcher takes its numbers from pc_set_shape_of.  Host only, no device code; the constants come from pc_pairs.h, the column kernel's
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
