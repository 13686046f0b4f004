// pc_common.h -- internal declarations shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PC_OPEN 11            // gap open   (metrics.py:160 default, parasail convention: first gap residue costs OPEN)
#define PC_EXT 1              // gap extend
#define PC_NEG (-(1 << 29))   // "-infinity" that survives a few subtractions without wrapping
#define PC_PADCODE 255        // residue code of padding: never equal to a real code
// Max alignments (row sequences) per workgroup task.  A wave of the systolic kernel keeps at most 64
// rows; rows are dealt to 4*nseg slots, so a wave receives ceil(R / (4 nseg)) * nseg of them: 208 is the
// largest R for which that is <= 64 for every nseg in 1..16.
#define PC_TASK_ROWS 208
#define PC_TASK_BUDGET 49152          // cell slots per row stream of a task (pc_nw_task_rows)
#define PC_MAX_W 64           // widest systolic variant: 64 lanes * 64 columns = 4096 columns

// Device view of the uploaded genomes (all pointers are HBM).
struct PcDev {
    int32_t N, Wb, Wstride, G;       // genomes, bitmap words per row, row stride in u64 (odd), genes
    int32_t U, ubits;                 // distinct gene sequences; bits of a sequence rank (2^ubits >= U)
    int32_t n_cu, pad_;               // compute units of the device these pointers live on (host-side grid sizing)
    int64_t E;                        // (genome, pham) entries
    const uint64_t* bitmap;           // [N][Wstride]
    const uint32_t* rankpre;          // [N][Wb]   entry index of the first set bit of word w of genome g
    const int32_t* ent_cnt;           // [E] genes of the genome in that pham
    const int32_t* ent_len;           // [E] their summed length
    const uint2* ent_pair_len;        // [E] (pham, summed length) and
    const uint2* ent_pair_cnt;        // [E] (pham, gene count): one 8-byte load per entry for k_sparse_tile
    // k_sparse_tile64's lists: entries of phams with at least two holders only, ids renumbered densely (sp_W 64-id words)
    const uint32_t* sp_end;           // [N] a genome's kept entries are [ent_off[g], sp_end[g]) of the three arrays below
    const int32_t* sp_pham;           // [E] dense id
    const uint2* sp_len;              // [E] (dense id, summed length)
    const uint2* sp_cnt;              // [E] (dense id, gene count)
    const uint32_t* sp_rank;          // [N][sp_W] first kept entry of the genome at or after dense word w
    int sp_W;
    const int32_t* ent_gene;          // [E] first gene id (genes of an entry are consecutive)
    const int32_t* ent_pham;          // [E] pham id (ascending within a genome: the set bits of its bitmap row, in order)
    const uint32_t* ent_off;          // [N+1] entries of genome g = [ent_off[g], ent_off[g+1])
    const uint32_t* para_off;         // [N+1] paralog entries of genome g (entries with more than one gene), ascending pham id:
    const int32_t* para_pham;         // [..] their pham id
    const int32_t* para_ex;           // [..] gene count - 1
    const int32_t* gene_len;          // [G]
    const int64_t* gene_off;          // [G] byte offset of the gene's codes (16-byte aligned)
    const uint8_t* codes;             // encoded residues, each gene padded to 16 B with PC_PADCODE
    const int32_t* nph;               // [N]
    const int32_t* ngen;              // [N]
    const int64_t* tlen;              // [N]
    const uint32_t* gene_q;           // [G] rank of the gene's sequence among the distinct sequences, in launch-class order
    const int32_t* q_gene;            // [U] a gene that carries sequence q (its first occurrence)
};

// Static shard: the target genomes this rank owns, ascending.
struct PcShard {
    int32_t nown;
    int32_t ident;                    // 1: owned[k] == k for every k (an unsharded context): kernels skip the table read
    const int32_t* owned;             // [nown] target genome t
    const int64_t* lbase;             // [nown+1] shard-local index of pair (0, owned[k]); pair (s,t) -> lbase[k] + s
};

// Pair domain of a rows fill: the query genomes, strictly ascending, against every other genome (k_walk_rows).
struct PcRows {
    int32_t nrows;
    const int32_t* rows;              // [nrows] query genome q
    const int32_t* row_of;            // [N] position of genome g in rows, or -1
};

// Pair domain of one slab of a rows slab fill (pc_fill_rows_edges / _components / _tree): vals = f64[m][n] as pc_fill_rows_dev lays it
// out, value i the pair {q = rows[i / n], g = i % n} -- source the smaller, target the larger -- and LIVE iff g != q and not
// (is_query[g] and g < q): the diagonal is no pair, and a pair of two query genomes is taken once, in the row of the smaller one,
// across all slabs of the call (is_query covers every query row of the CALL).  The passes see the slab flat, as the triangular ones
// do; a thread carries (row, column) of its elements by adds and a carry (PcRowsDomain, pc_slab_pass.h), adv_* being the launcher's
// stride between a thread's iterations.
struct PcRowsSlab {
    int32_t m, n;                     // the slab's rows; N
    const int32_t* rows;              // [m] query genome of row r, ascending
    const uint8_t* is_query;          // [n] 1: the genome is a query row of the call
    int32_t adv_rows, adv_cols;       // stride / n, stride % n (set by the launcher)
};
// Which pairs the values of a filled slab are, as the launchers of the slab passes take it: a triangular slab's shard or a rows slab's
// domain.  The converting constructors are meant: a description's slab() and the launchers are handed a PcShard or a PcRowsSlab as it is.
struct PcSlabDomain {
    bool is_rows; PcShard shard; PcRowsSlab rows;
    PcSlabDomain(const PcShard& s) : is_rows(false), shard(s), rows{} {}
    PcSlabDomain(const PcRowsSlab& r) : is_rows(true), shard{}, rows(r) {}
};

// Pair domain of a groups fill: every pair of two positions p < q of one group, over the members of a family of groups laid
// end to end (k_walk_groups).  Members ascend inside a group, so the genome at p is the pair's source and the one at q its target.
#define PC_GROUP_TILE 32      // positions per tile edge: the walkers' TS (pc_pairs.h), named here for the host units that list the tiles
struct PcGroups {
    int32_t M, pad_;                  // positions (members over all groups)
    const int32_t* pos_genome;        // [M] genome at position p
    const int32_t* pos_end;           // [M] end position of p's group: slot (p, q) is live iff p < q < pos_end[p]
    const int64_t* pos_rowbase;       // [M+1] output index of p's first pair; slot (p, q) = pos_rowbase[p] + q - p - 1; [M] = L
    const int32_t* tile_row;          // [T] the live TS x TS tiles over positions (row block a, column block b >= a), sorted by a, then b
    const int32_t* tile_col;          // [T]
    int64_t slot_base;                // first slot the na / off arrays of this launch hold (a range of row blocks is a range of slots)
};

// Pair domain of a pair-list fill: L slots, the caller's list sorted by (target, source) on the device (k_walk_pairs).  Slot i is the
// ORIENTED pair with source genome src[i] and target genome tgt[i] -- whatever their index order -- and its value goes to out[at[i]],
// the entry's position in the caller's list.  src[i] == tgt[i] is the diagonal: a dead slot, no alignment and no visit.
#define PC_PAIR_BLOCK 256     // slots per workgroup of k_walk_pairs: the unit a pair-list fill is cut by
struct PcPairs {
    int64_t L;                        // slots
    const int32_t* src;               // [L] source genome
    const int32_t* tgt;               // [L] target genome
    const uint32_t* at;               // [L] the caller's index of the entry
    int64_t slot_base;                // first slot the na / off arrays of this launch hold (a range of blocks is a range of slots)
};

// One wave task of the alignment kernels: column gene + a range of its bucket.
struct PcTask { int32_t gene, begin, end, pad; };   // pad: launch class of the task (planning only)

// Launch mode of a task, by how many of the workgroup's waves its rows can occupy (pc_nw_task_mode).  A task's launch class is
// base class * PC_WAVE_MODES + mode, so the three modes of a base class are neighbours in the sorted task list and a mode with
// too few tasks for a launch of its own is simply launched together with the one before it.
enum { PC_MODE_CLASS = 0, PC_MODE_TWO_WAVES = 1, PC_MODE_ONE_WAVE = 2, PC_WAVE_MODES = 3 };

// Per distinct column sequence q: how its bucket is cut into tasks.
struct PcTaskPlan {
    const int32_t* task_rows;         // [U] rows per task of the main variant
    const uint8_t* q_class;           // [U] launch class (variant * 4 + lanes-per-segment bucket) of the main tasks
    const uint8_t* q_nseg;            // [U] segments per wave of the main variant
    const uint8_t* rem_class;         // [U][16] launch class for a remainder of r rows (r = n mod nseg), 255: keep them in the main task
    int32_t nvar, small_modes;        // systolic variants; 1: tasks of at most nseg / 2 nseg rows get the one- / two-wave modes
    int32_t n_strip, pad_;            // strip-mined base classes (they follow the 2 x nvar x 4 systolic ones)
    int32_t variant_w[32];            // columns per lane of variant v
};

// walker modes (pc_walk.hip)
enum { PCW_POCP = 0, PCW_AF = 1, PCW_COUNT = 2, PCW_ENUM = 3, PCW_AAI = 4, PCW_PEQ = 5,
       PCW_GCS = 6, PCW_JC = 7,                     // these two: k_walk_rows / k_walk_groups / k_walk_pairs only (whole fills count gcs / jc on the tile kernels)
       PCW_JOINT = 8 };                             // k_walk (condensed) / k_walk_pairs only: PEQ's walk, up to six metrics of the pair out of it (PcJointArgs)
enum { PCW_SPARSE_GCS = 10, PCW_SPARSE_JC = 11 };   // k_sparse_tile64 only: shared-pham counts, one direction

struct PcWalkArgs {
    // COUNT
    uint32_t* na;                     // [Lp] alignments per pair
    unsigned long long* totals;       // [0] alignments [1] cells [2] residue bytes (as the reference would run them)
    unsigned long long* cost_t;       // [N] or NULL: DP cells per target genome (input of the cost-balanced deal)
    unsigned long long* aln_t;        // [N] or NULL: alignments per target genome (where a fill that exceeds its memory budget is cut);
                                      //   k_walk_rows: [nrows], alignments per query row (aln_row); k_walk_groups: per row block of positions;
                                      //   k_walk_pairs: per block of PC_PAIR_BLOCK slots
    // ENUM: alignment slot k of a pair = off[pair] + its position in the reference's loop order
    const uint32_t* off;              // [Lp] exclusive scan of na   (k_walk_rows: na / off are [rows of the range][N], slot (k - kb) * N + g;
                                      //   k_walk_groups, k_walk_pairs: the range's slots, slot - slot_base)
    unsigned long long* key;          // [A] (column sequence rank << ubits) | row sequence rank
    uint32_t* val;                    // [A] k
    // AAI / PEQ
    const uint32_t* alias;            // [A] slot -> index of its distinct (row sequence, column sequence) alignment
    const uint2* res;                 // [distinct alignments] (n_ident, aln_len)
    // output (POCP, AF, AAI, PEQ)
    double* out;
    int as_distance;
    int condensed;                    // 1: scipy condensed index, 0: shard-local index
};

// JOINT: the walk arguments of PEQ (out is not read) and, beside them, where each metric of the launch's set goes: metric m of the
// enum pc_metric (PC_GCS ... PC_PEQ) is written iff bit m of mask is set, to jout[m] -- at the index a.out would be written at.  Only
// the joint instantiations take this struct: the other kernels' parameters stay PcWalkArgs as it is.
struct PcJointArgs : PcWalkArgs {
    double* jout[6];
    uint32_t mask;
};

const char* pc_hip_err(hipError_t e);
void pc_set_error(const char* fmt, ...);

#define PC_HIP(call)                                                                            \
    do {                                                                                        \
        hipError_t _e = (call);                                                                 \
        if (_e != hipSuccess) { pc_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); return PC_ERR_HIP; } \
    } while (0)

// The set metrics' kernel families (pc_set_family of the C-ABI; pc_last_set_kernel) and their launch shapes.  pc_set_shape_of is the one
// statement of every launcher's arithmetic (pc_set_shape.hip): tile and super-tile edge, grid, units per workgroup, mask chunks, instance,
// seg / runs, LDS, epilogue table.  It reads nothing but its arguments; the launchers pass it the knobs they read from the environment.
enum { K_POPC, K_SPARSE32, K_SPARSE64, K_WALKER, K_SPARSE_COL };
struct pc_set_shape;
struct PcSetKnobs { int popc_tile, s64_chunks, col_seg; };        // PC_POPC_TILE, PC_S64_CHUNKS, PC_COL_SEG; 0: unset
PcSetKnobs pc_set_knobs_env();                                    // (read per launch: the tests switch them between fills)
// metric: PC_GCS ... PC_AF; sp_W: 64-id words of the phams with two holders; table_top: max_nph (gcs / jc) or max_ngen (pocp)
void pc_set_shape_of(int family, int metric, int N, int nown, int Wb, int sp_W, int n_cu, int table_top, const PcSetKnobs& knobs, pc_set_shape* out);
// which family fills a set metric: a function of its inputs alone (pc_set_shape.hip; pc_set_kernel_choice of the C-ABI)
struct pc_set_inputs;
int pc_set_choice(const pc_set_inputs& in);
// dimensions of the popcount tiles' epilogue table; false: too large (4 Mi entries), the division runs in place
bool pc_set_table_dims(int metric, int top, int* sh_dim, int* tot_dim);

// launchers (defined next to their kernels: pc_set_popc.hip, pc_walk.hip, pc_sparse.hip, pc_sparse_col.hip, pc_util.hip); shape_out: NULL or
// where the shape they launched with is left
int pc_launch_set_popc(const PcDev& d, const PcShard& sh, int metric, int as_distance, double* out, int condensed,
                       double* lut, bool build_lut, int top, hipStream_t st, pc_set_shape* shape_out = nullptr);
int pc_launch_walk(int mode, const PcDev& d, const PcShard& sh, const PcWalkArgs& a, hipStream_t st, pc_set_shape* shape_out = nullptr);
// the walker over the query rows [kb, ke) of a rows fill; a.out is the whole f64[nrows][N], a.condensed is not read
int pc_launch_walk_rows(int mode, const PcDev& d, const PcRows& rw, int kb, int ke, const PcWalkArgs& a, hipStream_t st);
// the walker over the tiles [tb, te) of a groups fill; a.out is the whole f64[L], a.condensed is not read
int pc_launch_walk_groups(int mode, const PcDev& d, const PcGroups& gr, int64_t tb, int64_t te, const PcWalkArgs& a, hipStream_t st);
// the walker over the blocks [bb, be) of PC_PAIR_BLOCK slots of a pair-list fill; a.out is the whole f64[L] in the caller's order,
// a.aln_t is per block, a.condensed is not read
int pc_launch_walk_pairs(int mode, const PcDev& d, const PcPairs& pr, int64_t bb, int64_t be, const PcWalkArgs& a, hipStream_t st);
// the JOINT walks: k_walk over the shard's pairs (condensed output only) and k_walk_pairs over the blocks [bb, be) of a pair list
int pc_launch_walk_joint(const PcDev& d, const PcShard& sh, const PcJointArgs& a, hipStream_t st);
int pc_launch_walk_pairs_joint(const PcDev& d, const PcPairs& pr, int64_t bb, int64_t be, const PcJointArgs& a, hipStream_t st);
// a pair list's sort: key[i] = tgt[i] << 32 | src[i], val[i] = i before pc_sort_pairs; src / tgt back out of the sorted keys after it
int pc_launch_pair_keys(const int32_t* src, const int32_t* tgt, unsigned long long* key, uint32_t* val, int64_t n, hipStream_t st);
int pc_launch_pair_split(const unsigned long long* key, int32_t* src, int32_t* tgt, int64_t n, hipStream_t st);
int pc_launch_sparse(int mode, const PcDev& d, const PcShard& sh, double* out, int as_distance, int condensed, hipStream_t st, pc_set_shape* shape_out = nullptr);   // pocp / af
int pc_launch_pair_entries(const int32_t* pham, const int32_t* len, const int32_t* cnt, uint2* pair_len, uint2* pair_cnt, int64_t n, hipStream_t st);
int pc_launch_sp_build(int N, const uint32_t* ent_off, const int32_t* pham, const int32_t* len, const int32_t* cnt, const int32_t* dense, int W2,
                       int32_t* sp_pham, uint2* sp_len, uint2* sp_cnt, uint32_t* sp_rank, uint32_t* sp_end, hipStream_t st);
int pc_launch_sparse64(int mode, const PcDev& d, const PcShard& sh, double* out, int as_distance, int condensed, hipStream_t st, pc_set_shape* shape_out = nullptr); // pocp / af, large matrices
// k_sparse_col (gcs / jc / pocp / af, large matrices): masks over a block of target genomes kept in LDS across a run of source tiles
size_t pc_sparse_col_lds(int mode, int P64);      // 0: the masks do not fit
int pc_sparse_col_vals_cap(int P64);             // pocp / af: entries (of phams with two holders) a block of 64 targets may hold
int pc_launch_sparse_col(int mode, const PcDev& d, const PcShard& sh, double* out, int as_distance, int condensed, hipStream_t st, pc_set_shape* shape_out = nullptr);
int pc_scan_exclusive_u32(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* tmp, int64_t tmp_elems, hipStream_t st);
int64_t pc_scan_tmp_elems(int64_t n);
// edge list of a filled slab (pc_edges.hip): chunks of the flat f64[Lp]; the elements per chunk that are pairs of dom (a rows slab:
// the LIVE ones, Lp = m * n) and pass; (s, t, value) of each at offs[chunk] + its rank within the chunk, in element order
int64_t pc_edge_chunks(int64_t Lp);
int pc_launch_edge_count(const double* vals, int64_t Lp, int as_distance, double thr, PcSlabDomain dom, uint32_t* counts, hipStream_t st);
int pc_launch_edge_emit(const double* vals, int64_t Lp, int as_distance, double thr, PcSlabDomain dom, const uint32_t* offs,
                        int32_t* src, int32_t* tgt, double* val, hipStream_t st);
// pc_fill_edges_bars: the predicate is pass(v, bar[s]) || pass(v, bar[t]); bar f64[N] on the device; a triangular slab (its shard) only
int pc_launch_edge_count_bars(const double* vals, int64_t Lp, int as_distance, const double* bar, const PcShard& sh, uint32_t* counts, hipStream_t st);
int pc_launch_edge_emit_bars(const double* vals, int64_t Lp, int as_distance, const double* bar, const PcShard& sh, const uint32_t* offs,
                             int32_t* src, int32_t* tgt, double* val, hipStream_t st);
int pc_rows_slab_span(int pass);                   // elements one workgroup of a slab pass covers (0: edges, 1: union, 2: tree scan; else 0)
// connected components of a filled slab's passing pairs (pc_components.hip): parent[g] = g and the pair counter zeroed; one slab's
// passing pairs hooked into parent[] (strict: < / > instead of <= / >=) and counted into *n_pass; labels[g] = root of g
int pc_launch_cc_init(int32_t* parent, int n, unsigned long long* n_pass, hipStream_t st);
int pc_launch_cc_union(const double* vals, int64_t Lp, int as_distance, int strict, double thr, PcSlabDomain dom, int32_t* parent,
                       unsigned long long* n_pass, hipStream_t st);
int pc_launch_cc_labels(int32_t* parent, int32_t* labels, int n, hipStream_t st);
// the forests of other devices united into parent[] (pc_multi_fill_components): fparent[n_foreign][n], each a forest k_cc_union left
int pc_launch_cc_merge(int32_t* parent, const int32_t* fparent, int n_foreign, int n, hipStream_t st);
// nearest neighbours of a filled slab (pc_nearest.hip): key[N * K] / nbr[N * K] set to the worst sentinel; the pairs of the slab of
// targets [t0, t1) merged into the K slots of every genome they touch (the row pass, then the column pass); values back from the keys
int pc_launch_nn_init(unsigned long long* key, int32_t* nbr, int64_t n, hipStream_t st);
int pc_launch_nn_select(const double* vals, int64_t Lp, int t0, int t1, int as_distance, int K, unsigned long long* key, int32_t* nbr, hipStream_t st);
int pc_launch_nn_select_rows(const double* vals, int64_t Lp, const PcRowsSlab& dom, int as_distance, int K, unsigned long long* key, int32_t* nbr,
                             hipStream_t st);
int pc_nn_seed_pack(const int32_t* seed_nbr, const double* seed_val, int k_seed, int ks, int N, int K, const uint8_t* is_query, int as_distance,
                    unsigned long long* key, int32_t* idx, int* bad_g, int* bad_j);
int pc_nn_rows_tile(void);
int pc_launch_nn_finish(const unsigned long long* key, double* val, int64_t n, int as_distance, hipStream_t st);
// k-nearest lists of a pair list (pc_nearest_of_pairs): src / tgt / val [L] on the device, L <= 2^30.  dkey / dpos [2 L]: every pair
// from both ends, key = owner << 32 | other, the pair's position behind it; after the caller's sort (skey / spos) start[N + 1] takes where
// each owner's run begins, and one wave per owner selects: key / nbr [N][K] best first, slots beyond count[g] = the run's length padded
// (nbr -1, the key of a quiet NaN: k_nn_finish then delivers NaN)
int pc_launch_nn_pair_entries(const int32_t* src, const int32_t* tgt, unsigned long long* dkey, uint32_t* dpos, int64_t L, hipStream_t st);
int pc_launch_nn_of_pairs(const unsigned long long* skey, const uint32_t* spos, const double* val, int64_t L, int N, int as_distance, int K,
                          uint32_t* start, unsigned long long* key, int32_t* nbr, int32_t* count, hipStream_t st);
// the lists of other devices merged into key / nbr [N][K] (pc_multi_fill_nearest): fkey / fnbr [n_foreign][N][K], in key space
int pc_launch_nn_merge(unsigned long long* key, int32_t* nbr, const unsigned long long* fkey, const int32_t* fnbr, int n_foreign, int N, int K, hipStream_t st);
// single-linkage tree of a filled slab (pc_tree.hip).  A pair's place in the total order is one word (the C-ABI header states it):
// key = micro << 44 | t << 22 | s, PC_TREE_NONE is no key.  A forest ("list") is u64[N + PC_TREE_TAIL]: at most N - 1 keys, then from
// word N - 1 its three tail words -- the number of keys, the values found outside the key's domain, the rounds that did work.
#define PC_TREE_NONE (~0ull)
#define PC_TREE_MICRO_MAX 1000000
#define PC_TREE_TAIL 2                             // words a list holds beyond its N: [N - 1] count, [N] violations, [N + 1] live rounds
__host__ __device__ inline unsigned long long pc_tree_key_of(int micro, int s, int t) {
    return ((unsigned long long)(uint32_t)micro << 44) | ((unsigned long long)(uint32_t)t << 22) | (unsigned long long)(uint32_t)s;
}
__host__ __device__ inline int pc_tree_key_micro(unsigned long long key) { return (int)(key >> 44); }
__host__ __device__ inline int pc_tree_key_t(unsigned long long key) { return (int)((key >> 22) & 0x3fffffu); }
__host__ __device__ inline int pc_tree_key_s(unsigned long long key) { return (int)(key & 0x3fffffu); }
int pc_tree_round_count(int n);                    // rounds enqueued per pass: max(1, ceil(log2 n))
// `out` takes over `in`'s violation and round counts (in == NULL: zeros) and is emptied; comp / best / live set for a pass's first round
int pc_launch_tree_reset(int32_t* comp, unsigned long long* best, uint32_t* live, int rounds, const unsigned long long* in,
                         unsigned long long* out, int n, hipStream_t st);
// the counts of n_foreign staged lists (each n + PC_TREE_TAIL words) added to `out`'s
int pc_launch_tree_take_counts(unsigned long long* out, const unsigned long long* lists, int n_foreign, int n, hipStream_t st);
// round r of a pass, in four steps: the slab's pairs and any number of lists lower best[], the roots hook and append to `out`, comp[] is
// flattened and best[] reset.  live: [rounds + 1]
int pc_launch_tree_scan_slab(const double* vals, int64_t Lp, int as_distance, PcSlabDomain dom, const int32_t* comp, unsigned long long* best,
                             unsigned long long* out, int n, const uint32_t* live, int r, hipStream_t st);
int pc_launch_tree_scan_list(const unsigned long long* list, const int32_t* comp, unsigned long long* best, int n, const uint32_t* live, int r,
                             hipStream_t st);
int pc_launch_tree_hook(const int32_t* comp, int32_t* next, const unsigned long long* best, unsigned long long* out, int n, uint32_t* live, int r,
                        hipStream_t st);
int pc_launch_tree_flatten(int32_t* comp, const int32_t* next, unsigned long long* best, unsigned long long* out, int n, const uint32_t* live, int r,
                           hipStream_t st);
// between-groups table of a filled slab (pc_between.hip).  The accumulator of G groups is one allocation of pc_between_bytes(G):
// sum u64[G][G] | cnt u64[G][G] | lo u32[G][G] | hi u32[G][G] | the 8-byte count of values that are no millionth in [0, 1].  Entry
// [group[t]][group[s]] takes pair (s, t); an empty accumulator is all zero but lo = ~0.  The folded result has the same layout with
// i64 / i64 / i32 / i32 arrays, symmetric.
#define PC_BETWEEN_SEGMENT 4096                    // elements of a slab row one workgroup of k_between_rows takes
struct PcBetweenAcc { unsigned long long *sum, *cnt; uint32_t *lo, *hi; unsigned long long* bad; };
static inline size_t pc_between_bytes(int G) { return (size_t)G * (size_t)G * 24 + 8; }
__host__ __device__ static inline PcBetweenAcc pc_between_view(void* base, int G) {
    const size_t gg = (size_t)G * (size_t)G;
    unsigned long long* const sum = (unsigned long long*)base;
    uint32_t* const lo = (uint32_t*)(sum + 2 * gg);
    return PcBetweenAcc{sum, sum + gg, lo, lo + gg, (unsigned long long*)(lo + 2 * gg)};
}
int pc_launch_between_init(void* acc, int G, hipStream_t st);
// one slab: vals f64[Lp] in the shard's layout, max_row its longest row; group: [N] on the device, every label in [0, G)
int pc_launch_between_rows(const double* vals, int64_t Lp, const PcShard& sh, int64_t max_row, const int32_t* group, int G, void* acc, hipStream_t st);
// one rows slab (dom: f64[m][n] at vals): the live elements of every query row with a label; group: [N] on the device, every label in [-1, G)
int pc_launch_between_qrows(const double* vals, int64_t Lp, const PcRowsSlab& dom, const int32_t* group, int G, void* acc, hipStream_t st);
// the accumulators of other devices added into acc: staged[n_foreign] of pc_between_bytes(G) each
int pc_launch_between_merge(void* acc, const void* staged, int n_foreign, int G, hipStream_t st);
// the square made symmetric into out (the result layout), empty entries as lo = INT32_MAX, hi = -1; invert: the accumulator holds
// distances and out takes the similarity table, every millionth's complement
int pc_launch_between_fold(const void* acc, void* out, int G, int invert, hipStream_t st);
// histogram of a filled slab's pair values (pc_hist.hip).  The state of `classes` classes (1: no partition; 2: within, between) is one
// allocation of pc_hist_bytes(classes): u64 hist[classes][PC_HIST_BINS] | the 8-byte count of values that are no millionth in [0, 1].
// Bin k of a class counts its pairs of micro k; an empty state is all zero.  The finished result has the same layout, i64.
#define PC_HIST_BINS 1000001
static inline size_t pc_hist_bytes(int classes) { return ((size_t)classes * PC_HIST_BINS + 1) * 8; }
int pc_hist_table_slot_count(void);                // slots of the pass's LDS table
int pc_hist_probe_bound(void);                     // slots an insert tries before it goes to the global bin
// one slab (either pair domain); group: [N] on the device, every label compared only, or NULL (classes == 1)
int pc_launch_hist_pass(const double* vals, int64_t Lp, PcSlabDomain dom, const int32_t* group, int classes, void* state, hipStream_t st);
// the states of other devices added into state: staged[n_foreign] of pc_hist_bytes(classes) each
int pc_launch_hist_merge(void* state, const void* staged, int n_foreign, int classes, hipStream_t st);
// the state into out (the result layout); invert: the state holds distances and out takes the similarity histogram, every class reversed
int pc_launch_hist_finish(const void* state, void* out, int classes, int invert, hipStream_t st);
// genome x group table of a filled slab (pc_affinity.hip).  The resident table of N genomes and G groups is one allocation of
// pc_affinity_table_bytes(N, G): PcAffinityEntry[N][G] | the 8-byte count of values that are no millionth in [0, 1].  Entry [g][b]
// takes the pairs of g with the members of b; an empty entry is (0, ~0, 0).  The result (PcAffinityOut over one allocation of
// pc_affinity_out_bytes) is the violation count, the O(N) arrays and, when wanted, the converted table behind them.
#define PC_AFFINITY_BLOCK 64                       // consecutive sources one wave of k_aff_cols takes, a lane each
struct PcAffinityEntry { unsigned long long sum; uint32_t lo, hi; };
static_assert(sizeof(PcAffinityEntry) == 16, "16 bytes per entry");
static inline size_t pc_affinity_table_bytes(int N, int G) { return (size_t)N * (size_t)G * sizeof(PcAffinityEntry) + 8; }
struct PcAffinityOut {
    unsigned long long* bad;
    long long *own_sum, *near_sum;                  // [N]
    int32_t *own_lo, *own_hi, *near_group, *near_lo, *near_hi;   // [N]; near_group: [3][N], by mean, by minimum, by maximum
    long long* tab_sum; int32_t *tab_lo, *tab_hi;   // [N][G], or NULL: the table was not asked for
};
static inline size_t pc_affinity_head_bytes(int N) { return ((size_t)8 + (size_t)N * 44 + 7) & ~(size_t)7; }
static inline size_t pc_affinity_out_bytes(int N, int G, int want_table) {
    return pc_affinity_head_bytes(N) + (want_table ? (size_t)N * (size_t)G * 16 : 0);
}
static inline PcAffinityOut pc_affinity_out_view(void* base, int N, int G, int want_table) {
    const size_t n = (size_t)N, ng = n * (size_t)G;
    PcAffinityOut o{};
    o.bad = (unsigned long long*)base;
    o.own_sum = (long long*)(o.bad + 1); o.near_sum = o.own_sum + n;
    o.own_lo = (int32_t*)(o.near_sum + n); o.own_hi = o.own_lo + n; o.near_group = o.own_hi + n; o.near_lo = o.near_group + 3 * n; o.near_hi = o.near_lo + n;
    if (want_table) {
        o.tab_sum = (long long*)((char*)base + pc_affinity_head_bytes(N));
        o.tab_lo = (int32_t*)(o.tab_sum + ng); o.tab_hi = o.tab_lo + ng;
    }
    return o;
}
int pc_launch_affinity_init(void* tab, int N, int G, hipStream_t st);
// one slab of the consecutive targets [t0, t0 + sh.nown): vals f64[Lp] in the shard's layout; group / member / goff on the device, every
// label in [0, G); grange: [n_ranges + 1] group ranges of the column pass, ascending from 0 to G
int pc_launch_affinity_rows(const double* vals, int64_t Lp, const PcShard& sh, int t0, int N, const int32_t* group, int G, void* tab, hipStream_t st);
int pc_launch_affinity_cols(const double* vals, int64_t Lp, const PcShard& sh, int t0, int N, const int32_t* member, const int32_t* goff,
                            const int32_t* grange, int n_ranges, int G, void* tab, hipStream_t st);
// the tables of other devices combined into tab: staged[n_foreign] of pc_affinity_table_bytes(N, G) each
int pc_launch_affinity_merge(void* tab, const void* staged, int n_foreign, int N, int G, hipStream_t st);
// the result into out (pc_affinity_out_bytes); invert: the table holds distances and out takes the similarity statement
int pc_launch_affinity_finish(const void* tab, const int32_t* group, const int32_t* goff, int N, int G, int invert, void* out, int want_table, hipStream_t st);
// The rows form (pc_fill_rows_affinity): n_rows query genomes against the groups.  The resident state is one allocation of
// pc_affinity_rows_state_bytes: PcAffinityEntry[n_rows][G] (row k the query rows[k]) | PcAffinityEntry gain[N] (what the queries add to an
// old genome's own entry; used with want_gain only) | the 8-byte violation count.  The result is PcAffinityOut over n_rows rows
// (pc_affinity_out_bytes(n_rows, G, want_table)) with, want_gain only, PcAffinityGainOut over N genomes behind it (16 N bytes).
struct PcAffinityGainOut { long long* sum; int32_t *lo, *hi; };      // [N]; all NULL: the gain was not asked for
static inline size_t pc_affinity_rows_entries(int n_rows, int N, int G) { return (size_t)n_rows * (size_t)G + (size_t)N; }
static inline size_t pc_affinity_rows_state_bytes(int n_rows, int N, int G) { return pc_affinity_rows_entries(n_rows, N, G) * sizeof(PcAffinityEntry) + 8; }
static inline size_t pc_affinity_rows_out_bytes(int n_rows, int N, int G, int want_table, int want_gain) {
    return pc_affinity_out_bytes(n_rows, G, want_table) + (want_gain ? (size_t)N * 16 : 0);
}
static inline PcAffinityGainOut pc_affinity_gain_view(void* base, int n_rows, int N, int G, int want_table, int want_gain) {
    PcAffinityGainOut o{};
    if (want_gain) {
        o.sum = (long long*)((char*)base + pc_affinity_out_bytes(n_rows, G, want_table));
        o.lo = (int32_t*)(o.sum + (size_t)N); o.hi = o.lo + (size_t)N;
    }
    return o;
}
// every entry of the state empty, the count 0
int pc_launch_affinity_rows_init(void* state, int n_rows, int N, int G, hipStream_t st);
// one rows slab (dom: f64[m][N] at vals, query rows r0 .. r0 + m of the call): k_aff_qrows, and with want_gain k_aff_qcols behind it; group on
// the device, every label in [-1, G).  *between, when not NULL, is recorded between the two launches
int pc_launch_affinity_rows_slab(const double* vals, int64_t Lp, const PcRowsSlab& dom, int r0, int n_rows, const int32_t* group, int G, void* state,
                                 int want_gain, hipEvent_t between, hipStream_t st);
// the result into out (pc_affinity_rows_out_bytes); rows[n_rows], goff[G + 1] (the labelled genomes of each group) and qcount[G] (the
// query genomes among them) on the device
int pc_launch_affinity_rows_finish(const void* state, const int32_t* rows, const int32_t* group, const int32_t* goff, const int32_t* qcount, int n_rows, int N,
                                   int G, int invert, void* out, int want_table, int want_gain, hipStream_t st);
// residue bytes -> codes on the device (pc_plan.hip): gene k's raw bytes [seq_off[k], seq_off[k+1]) go through the LUT to
// codes + gene_off[k], padded with PC_PADCODE to a multiple of 16
struct PcLut { uint8_t v[256]; };
int pc_launch_encode(const uint8_t* raw, const int64_t* seq_off, const int64_t* gene_off, const int32_t* gene_len, const PcLut& lut,
                     uint8_t* codes, int G, hipStream_t st);
// planning of the alignment batch (pc_plan.hip)
int pc_launch_task_keys(const PcDev& d, const PcTask* tasks, unsigned long long* key, uint32_t* val, int ntasks, hipStream_t st);
int pc_launch_task_gather(const PcTask* in, const uint32_t* idx, PcTask* out, int ntasks, hipStream_t st);
size_t pc_sort_temp_bytes(int64_t n, int bits);
int pc_sort_pairs(void* temp, size_t temp_bytes, const unsigned long long* key_in, unsigned long long* key_out, const uint32_t* val_in,
                  uint32_t* val_out, int64_t n, int bits, hipStream_t st);
int pc_launch_mark_heads(const unsigned long long* skey, uint32_t* flags, int64_t n, hipStream_t st);
int pc_launch_unique(const PcDev& d, const unsigned long long* skey, const uint32_t* sval, const uint32_t* flags, const uint32_t* excl,
                     uint32_t* alias, int32_t* bucket_row, uint32_t* start_q, uint32_t* end_q, unsigned long long* totals, int64_t n, hipStream_t st);
int pc_launch_task_count(const uint32_t* start_q, const uint32_t* end_q, const PcTaskPlan& tp, uint32_t* ntask_q, int U, hipStream_t st);
int pc_launch_task_fill(const PcDev& d, const uint32_t* start_q, const uint32_t* end_q, const PcTaskPlan& tp, const uint32_t* task_off_q,
                        PcTask* tasks, int U, hipStream_t st);
int pc_launch_class_bounds(const unsigned long long* sorted_key, int ntasks, int ncls, uint32_t* cls_begin /*[ncls+1]*/, hipStream_t st);
int pc_launch_task_slice(const PcTask* sorted, int ntasks, const uint32_t* cls_begin, const uint32_t* slice_begin /*[ncls+1]*/, int rank, int world,
                         PcTask* out, hipStream_t st);   // every world-th task of each class from `rank`, compacted
int pc_launch_gather_u32(const uint32_t* src, const int32_t* idx, uint32_t* dst, int n, hipStream_t st);
int pc_launch_assemble(const double* gathered, int world, int64_t stride, int N, double* out, hipStream_t st);
int pc_launch_assemble_table(const double* gathered, int64_t stride, int N, const int32_t* t_rank, const int64_t* t_lbase, double* out, hipStream_t st);
int pc_launch_round6_probe(const double* in, double* out, int64_t n, hipStream_t st);
int pc_launch_unpack_res(const uint2* res, const int32_t* la_plus_lb, int32_t* n_ident, int32_t* n_diag, int64_t n, hipStream_t st);

// K4's launch arithmetic (pc_nw_shape.hip: host only, no device code; the geometry it shares with the kernels: pc_nw_geometry.h)
int pc_nw_num_variants();
int pc_nw_variant_w(int v);                       // columns per lane of variant v
int pc_nw_choose_variant(int lb);                 // -1: general fallback
// compare_only: the launch class is the one for column genes holding a byte outside the 24-letter alphabet, which must run
// the residue-compare cell (the profile cell keeps ONE row for all such bytes: exact only while the column holds none)
int pc_nw_class_waves(int variant, int lb, int compare_only);   // waves per workgroup of the launch class a column gene of lb residues falls in
int pc_nw_variant_takes_any_byte(int v);          // 0: the variant has classes that run the profile cell, so such column genes need the compare_only classes
int pc_nw_task_rows(int lb, int variant, int compare_only);     // rows per workgroup task for that column gene
int pc_nw_ppos_systolic(int variant, int max_lb); // 1: a percent-positives launch of this class can run on the systolic kernel (its profile cell)
int pc_nw_ppos_variant(int max_lb);               // the variant to run it on when the class's own cannot; -1: general kernel
int pc_nw_choose_remainder(int lb, int r, int main_variant);   // variant for a bucket's last r < nseg rows, -1: keep them
int pc_nw_task_mode(int lb, int rows, int variant);            // PC_MODE_* of a task of `rows` rows on that variant
int pc_nw_small_modes_enabled();
// several launch classes in ONE launch (k_nw_systolic_tier): classes whose pc_nw_fuse_key agrees (and is >= 0) may share it
int pc_nw_fuse_key(int variant, int max_lb, int ppos, int compare_only, int wave_mode);
size_t pc_nw_strip_scratch_bytes(int max_row_len, int n_cu);    // scratch a strip-mined launch (max_lb > 64 x W of its variant) wants
size_t pc_nw_strip_launch_bytes(int wave_mode, int ntasks, int max_row_len, int n_cu, int ppos);   // ... and one such launch with a region of its own
int pc_nw_launch_is_strip(int variant, int max_lb, int wave_mode, int ppos);   // the launch runs on k_nw_strip and needs the scratch slab
int pc_nw_strip_passes(int lb, int variant);                   // passes of 64 x W columns a column gene of lb residues takes on that variant (1: not strip-mined)
size_t pc_nw_fallback_scratch_bytes(int max_lb);
// Shape of ONE systolic or strip-mined launch, as the launchers (pc_nw.hip) take it: the width to instantiate and its cell, waves per
// workgroup, dynamic LDS; strip: it runs on k_nw_strip, pipe: in the form that deals one alignment's passes over the waves, per_cu:
// the resident workgroups per CU its scratch is sized for (0: not strip-mined).  ntasks, n_cu: read for strip-mined launches only.
struct PcLaunchShape { int W, nw; bool inc16, strip, pipe; size_t lds; int per_cu; };
int pc_nw_launch_shape(int variant, int max_lb, int ppos, int compare_only, int wave_mode, int ntasks, int n_cu, PcLaunchShape& sh);

// The launch classes.  Base class of a column gene: variant * 4 + bucket of lanes per segment (<=8, <=16, <=32, <=64); the same again,
// nvar * 4 higher, for column genes that hold a byte outside the 24-letter alphabet ("any byte" classes: they must run
// the residue-compare cell, see above); then one class per wide variant for column genes longer than its 64 x W columns
// (strip-mined passes, k_nw_strip); last class: the general kernel.
#define PC_STRIP_CLASSES 3                                 // W = 32, 48, 64: the last three variants
int pc_num_classes();
int pc_class_of(int lb, int variant, bool any_byte);
int pc_class_variant(int cls);
int pc_class_compare_only(int cls);
// How a bucket of `rows` distinct rows against a column gene of lb residues is cut into tasks -- the host statement of the cut
// that pc_plan.hip makes on the device from the upload's tables (q_class, q_nseg, task_rows, rem_class): pc_align_pairs cuts its
// buckets with it and pc_bucket_launch_classes reports it.  base: the column gene's base class (pc_class_of of its variant);
// move_remainder: the left-over rows of a wave round may go to the remainder chooser's variant (the automatic variant only).
struct PcBucketCut { int per; int64_t n_main; int rem_base; };     // rows per main task, rows of the main tasks, base class of the remainder task (-1: none)
PcBucketCut pc_bucket_cut(int lb, int64_t rows, int base, bool any_byte, bool move_remainder);
// launch class of a task of `rows` rows of that bucket on base class `base`; modes: 0 = every task in its class's own workgroup shape (a forced variant)
int pc_task_launch_class(int lb, int rows, int base, bool modes);

// the alignment launchers (pc_nw.hip)
int pc_launch_nw(int variant, const PcDev& d, const PcTask* tasks, int ntasks, const int32_t* bucket_row,
                 const uint32_t* bucket_dest, uint2* res, void* scratch, size_t scratch_bytes, int max_lb, int ppos, int tie_rule, int compare_only, hipStream_t st,
                 int wave_mode = 0,    // wave_mode: PC_MODE_* -- workgroup shape of the launch's tasks
                 int max_row_len = 65535);   // longest row sequence (sizes a strip-mined launch's boundary lines; see pc_nw_strip_scratch_bytes)
#define PC_FUSE_MAX_SEGMENTS 32
struct PcNwSegment { uint32_t task_begin, ntasks; int variant, max_lb, compare_only, wave_mode; };
int pc_launch_nw_group(const PcNwSegment* segs, int nsegs, const PcDev& d, const PcTask* task_list, const int32_t* bucket_row,
                       const uint32_t* bucket_dest, uint2* res, int ppos, int tie_rule, hipStream_t st);
