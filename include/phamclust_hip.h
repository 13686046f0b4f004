/*
 * phamclust_hip.h -- C-ABI of libphamclust_hip.so: the MI355X (gfx950) implementation of
 * phamclust's pairwise genome-similarity matrix fill.
 *
 * The reference (chg60/phamclust, pure Python) has no FFI; the operator boundary this
 * library sits behind is
 *     matrix_de_novo(genomes, func, cpus, as_distance=True) -> SymMatrix
 *                                   /root/reference/src/phamclust/matrix.py:432-497
 *     METRICS = {"gcs","jc","pocp","af","aai","peq"} -> f(source, target, as_distance)
 *                                   /root/reference/src/phamclust/cli.py:30-35
 *                                   /root/reference/src/phamclust/metrics.py:26-253
 * The entry points below are what a ctypes binding for that boundary calls
 * (INTEGRATION.md shows the stub).  Plain pointers and sizes only; no exceptions or
 * aborts cross this boundary: every function returns 0 or a negative pc_status and
 * leaves a message for pc_last_error().
 *
 * Threading: one host thread drives one pc_ctx; one pc_ctx drives one GPU.  Multi-GPU, two ways:
 * one process per GPU (one ctx per rank + pc_set_shard*, the exchange is the caller's single
 * RCCL gather of the shard buffers), or one process for all of them (pc_multi_*: the library
 * owns a ctx and a host thread per device and does the exchange itself).
 */
#ifndef PHAMCLUST_HIP_H
#define PHAMCLUST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_VERSION 173   /* 0.5.22: pc_fill_joint, pc_fill_joint_dev, pc_fill_pairs_joint, pc_fill_pairs_joint_dev (all six metrics of a pair from one alignment pass) */

typedef enum {
    PC_OK = 0,
    PC_ERR_ARG = -1,        /* bad argument / inconsistent packed data          */
    PC_ERR_HIP = -2,        /* a HIP runtime call failed                         */
    PC_ERR_STATE = -3,      /* call order (e.g. fill before upload)              */
    PC_ERR_LIMIT = -4,      /* problem exceeds an implementation limit           */
    PC_ERR_DATA = -5        /* data the reference cannot process either (empty translation under aai/peq) */
} pc_status;

/* metric ids follow the order of the reference's METRICS dict (cli.py:30-35) */
typedef enum { PC_GCS = 0, PC_JC = 1, PC_POCP = 2, PC_AF = 3, PC_AAI = 4, PC_PEQ = 5,
               PC_AAI_PPOS = 6   /* average_aminoacid_identity(..., ppos=True), metrics.py:218-220: not a METRICS entry, no CLI route */
} pc_metric;

typedef struct pc_ctx pc_ctx;

/*
 * Packed genomes: host memory, caller-owned, read-only during pc_upload (the library
 * copies what it needs).  Genome order is the name-sorted list order of
 * scripts/phamclust.py:221 and fixes pair orientation: for s < t, s is the reference's
 * `source`, t its `target` (matrix.py:479-486).
 */
typedef struct {
    int32_t n_genomes;          /* N                                                       */
    int32_t n_phams;            /* P                                                       */
    int32_t words_per_row;      /* W = max(1, ceil(P/64))                                  */
    int32_t reserved;           /* must be 0                                               */
    const uint64_t* bitmap;     /* [N*W] bit (p & 63) of word (p >> 6) of row g: g holds pham p  (Genome.phams keys, genome.py:28) */
    const int32_t* nph;         /* [N] len(g.phams)                  (metrics.py:46)        */
    const int32_t* ngen;        /* [N] len(g)                        (genome.py:168-169)    */
    const int64_t* tlen;        /* [N] sum of len(translation)       (metrics.py:135-147)   */
    const int64_t* gene_off;    /* [N+1] genes of genome g = [gene_off[g], gene_off[g+1])   */
    const int32_t* gene_pham;   /* [G] ascending within a genome, paralogs in list order    */
    const int64_t* seq_off;     /* [G+1] residues of gene k = [seq_off[k], seq_off[k+1])    */
    const uint8_t* residues;    /* [R] raw bytes, one per character                         */
} pc_packed;

/* Filled by the fill calls when non-NULL.  Times are HIP-event milliseconds on the
 * stream the kernels ran on. */
typedef struct {
    int64_t n_pairs;            /* genome pairs produced by this call (this rank's shard)   */
    int64_t n_alignments;       /* alignments the reference would run (aai/peq), else 0     */
    int64_t n_cells;            /* sum of la*lb over those alignments                       */
    int64_t n_tasks;            /* wave tasks launched by the alignment kernels             */
    int64_t n_residue_bytes;    /* sum of (la+lb) over alignments: algorithmic input bytes  */
    int32_t n_align_launches;   /* alignment kernel launches                                */
    int32_t n_chunks;           /* plan -> align -> reduce passes the fill took (1 unless the plan exceeded the budget) */
    float ms_total;             /* whole call, device side                                  */
    float ms_plan;              /* pair walk: counts, scans, bucketing, task build          */
    float ms_align;             /* alignment kernels only (the dominant kernels)            */
    float ms_reduce;            /* best-match select + fp64 epilogue (or the set-metric kernel) */
    int64_t n_distinct_alignments; /* distinct (row sequence, column sequence) pairs: what the kernels computed */
    int64_t n_distinct_cells;   /* sum of la*lb over the distinct alignments                */
} pc_stats;

int pc_version(void);
const char* pc_last_error(void);
/* 1 in a library compiled with -DPC_TEST_HOOKS (libphamclust_hip_hooks.so: fault injection for the tests, see the knob table
 * at the end of this header), 0 in the release library. */
int pc_test_hooks(void);
/* Test hook, only in effect in libphamclust_hip_hooks.so (PC_VERSION 166): values, the whole triangle of the uploaded collection as
 * n_pairs = N (N - 1) / 2 doubles in the slab walk's own order -- target-major: element t (t - 1) / 2 + s is the pair (s, t), s < t --
 * stands for "the slab as filled" in every triangular slab walk of the process from now on: pc_fill_edges, _components, _nearest, _tree,
 * _between, _affinity, _hist and their pc_multi_ forms.  The fill still runs (the uploaded collection only sets N); each slab is then overwritten
 * with its stretch of the triangle by one host-to-device copy on the walk's stream, in whichever direction the fill ran: between, hist and
 * affinity always fill distances and invert at the end, the other four fill the direction asked for.  The pointer is stored process-wide,
 * not the values: the caller keeps the memory alive and unchanged until it clears the hook with values == NULL, and sets or clears it
 * between calls only.  A walk that finds n_pairs != N (N - 1) / 2 refuses with PC_ERR_ARG.  The rows walk (pc_fill_rows_edges,
 * _components, _tree, _nearest, _affinity, _between, _hist) does not read it: pc_hook_rows_values is its hook.  PC_ERR_ARG: values with a negative n_pairs.
 * In the release library: PC_ERR_STATE and an error text, with a pointer and with NULL alike; nothing is stored. */
int pc_hook_slab_values(const double* values, int64_t n_pairs);
/* Test hook, only in effect in libphamclust_hip_hooks.so (PC_VERSION 167): values, f64[n_rows][n], row k the values of the call's query
 * genome rows[k] to every genome, stands for "the slab as filled" in every rows walk of the process from now on: pc_fill_rows_edges,
 * _components, _tree, _nearest, _affinity, _between, _hist.  The rows fill still runs; each slab of m rows starting at query row r0 is then overwritten with
 * values + r0 * n, m * n doubles, by one host-to-device copy on the walk's stream -- EVERY element of it: the diagonal [k][rows[k]] and
 * both copies of a pair of two query genomes are the caller's too, so a test decides what the elements hold that no pass may read.
 * pc_fill_rows, pc_fill_rows_dev and the triangular walk do not read it; the two hooks are independent.  The pointer is stored
 * process-wide, not the values: the caller keeps the memory alive and unchanged until it clears the hook with values == NULL, and sets
 * or clears it between calls only.  A walk whose n_rows or N is not the hook's refuses with PC_ERR_ARG.  PC_ERR_ARG: values with a
 * negative n_rows or n.  In the release library: PC_ERR_STATE and an error text, with a pointer and with NULL alike; nothing is stored. */
int pc_hook_rows_values(const double* values, int32_t n_rows, int32_t n);

/* One context per GPU.  device_id is the HIP device ordinal. */
int pc_ctx_create(pc_ctx** out, int device_id);
void pc_ctx_destroy(pc_ctx* ctx);

/* Copy the packed genomes to HBM and build the device-side indices (rank table, gene
 * table, encoded residues).  Replaces any previous upload. */
int pc_upload(pc_ctx* ctx, const pc_packed* genomes);

/* The same in two parts.  gcs / jc / pocp / af read pham sets, gene counts and translation LENGTHS only
 * (metrics.py:26-157), and encoding, de-duplicating and ranking the residues is ~90 % of pc_upload's time:
 *   pc_upload_sets      bitmap, rank table, (genome, pham) entries, per-genome scalars -- enough for the four set metrics
 *                       and for pc_set_shard*; replaces any previous upload;
 *   pc_upload_residues  what aai / peq and pc_align_pairs need on top; `genomes` must be the packed genomes
 *                       pc_upload_sets was given (checked by size; the caller keeps them alive in between).  A no-op
 *                       when the residues are already there.
 * aai / peq fills before pc_upload_residues return PC_ERR_STATE. */
int pc_upload_sets(pc_ctx* ctx, const pc_packed* genomes);
int pc_upload_residues(pc_ctx* ctx, const pc_packed* genomes);

/*
 * Static shard of the upper-triangular pair list: rank r of `world` owns the pairs
 * (s, t), s < t, of the target genomes t it is dealt (boustrophedon deal over t, so the
 * linear cost ramp in t balances).  Default after upload: rank 0 of 1 = every pair.
 * pc_shard_pairs: pairs owned; pc_shard_stride: max over ranks (equal-count gather size).
 */
int pc_set_shard(pc_ctx* ctx, int rank, int world);

/* Same contract, cost-balanced deal: one device pass counts the alignment work (DP cells) behind every target genome,
 * then targets go, heaviest first, to the rank with the least work so far.  Deterministic, so every rank of a job
 * arrives at the same partition without communicating; use it on all ranks or on none (pc_assemble_dev follows the
 * deal that is in force).  Worth it when genomes differ in size or in how much they share. */
int pc_set_shard_balanced(pc_ctx* ctx, int rank, int world);
int64_t pc_shard_pairs(const pc_ctx* ctx);
int64_t pc_shard_stride(const pc_ctx* ctx);
/* The deal in force, for callers that assemble (or check) the gathered shards themselves: target genome t belongs to
 * rank t_rank[t] and pair (s, t), s < t, sits at index t_lbase[t] + s of that rank's shard.  Both arrays hold N entries. */
int pc_shard_table(const pc_ctx* ctx, int32_t* t_rank, int64_t* t_lbase);
/* DP cells behind each target genome (sum over s < t), as counted for the cost-balanced deal; N entries.
 * PC_ERR_STATE until pc_set_shard_balanced has run for the current upload. */
int pc_target_costs(const pc_ctx* ctx, uint64_t* cost);

/*
 * matrix_de_novo's fill (matrix.py:479-491) for the six METRICS, whole matrix, one GPU.
 * out_condensed: host f64[N(N-1)/2] in scipy condensed order (row-major strict upper
 * triangle) in packed-genome index space.  Values are already round(x, 6) exactly as
 * the reference returns them; the diagonal is not produced (matrix.py:467-468 presets it).
 */
int pc_fill(pc_ctx* ctx, int metric, int as_distance, double* out_condensed, pc_stats* stats);

/*
 * Memory-bounded batching of aai / peq fills (the reference bounds its in-flight work the same way: ~10,000 pairs per
 * CPU per batch, matrix.py:474-493).  The plan of a fill costs ~56 bytes of HBM per alignment; when that exceeds the
 * budget -- bytes, 0 = automatic: half of the HBM free at the time; environment PC_PLAN_BYTES at context creation -- or
 * the 2^31-2 alignments one plan can index, every fill entry point runs plan -> align -> reduce over successive ranges of
 * its target genomes (pc_stats.n_chunks passes) and produces the same values bit for bit.  A device allocation that fails
 * inside a fill is answered by halving the chunk, not by an error.  Only pc_plan_dev (the alignment-sliced route, which
 * keeps the whole plan resident) still refuses more than 2^31-2 alignments.
 */
int pc_set_plan_budget(pc_ctx* ctx, int64_t bytes);
/* The chunking rule itself, host arithmetic only (no GPU; exported for tests): cut count[0..n) into consecutive ranges
 * whose sums stay <= max_per_chunk (an element above it gets a range of its own).  chunk_begin receives the range starts
 * followed by n (at most cap entries are written); returns the number of ranges. */
int pc_chunk_plan(const uint64_t* count, int n, uint64_t max_per_chunk, int32_t* chunk_begin, int cap);

/* Same values, delivered in page-locked host memory owned by the context (grow-only, pinned once): *out_host points to
 * f64[N(N-1)/2] and stays valid until the next fill or upload on this context, or its destruction.  This is the call
 * matrix_de_novo uses: the result is expanded into the SymMatrix straight away, so nothing outlives the loan. */
int pc_fill_borrow(pc_ctx* ctx, int metric, int as_distance, const double** out_host, pc_stats* stats);

/* Same, result left in HBM: out_dev is a device pointer to f64[N(N-1)/2]; `stream` is a
 * hipStream_t; NULL is the legacy default stream, as everywhere in HIP (PyTorch's default stream has
 * handle 0: work the caller queued there is ordered with these launches).  Asynchronous w.r.t. the host except for
 * one small plan read-back under aai/peq. */
int pc_fill_dev(pc_ctx* ctx, int metric, int as_distance, void* out_dev, void* stream, pc_stats* stats);

/* This rank's shard only, shard-local order, into device memory f64[pc_shard_stride()]
 * (tail beyond pc_shard_pairs() is zero-filled).  Followed by the caller's RCCL gather. */
int pc_fill_shard_dev(pc_ctx* ctx, int metric, int as_distance, void* shard_dev, void* stream, pc_stats* stats);

/*
 * Rows fill: new genomes against a filled matrix.  The reference has the container half of this -- SymMatrix.append_node grows
 * a matrix by one node, matrix.py:169-213 -- and nothing that produces the values to feed it; its only fill is the whole
 * triangle (matrix.py:479-491).  `rows` holds n_rows distinct genome indices, strictly ascending (the "query" genomes); the
 * call fills the pairs {q, g}, q in rows, g != q, each in the whole fill's orientation -- min(q, g) is the reference's
 * `source`, max(q, g) its `target` -- and with the whole fill's values bit for bit, a pair of two queries computed once.
 * out: row-major f64[n_rows][N]: out[k * N + g] is the value of {rows[k], g}, out[k * N + rows[k]] the diagonal,
 * 1.0 - as_distance (matrix.py:467-468).  The six metrics and PC_AAI_PPOS.  gcs / jc / pocp / af always run on the rows
 * walker: no selector, and pc_last_set_kernel / pc_last_set_launch keep reporting the last whole fill.  aai / peq are cut
 * into successive ranges of rows under the rule of pc_set_plan_budget (the chunking rule over the rows' alignment counts; the
 * 8 bytes per slot of the per-pair count / offset arrays count against the budget, so only one range's slot arrays are ever
 * resident), same values whatever the cut.  stats: n_pairs = n_rows (N - 1) - n_rows (n_rows - 1) / 2 distinct pairs;
 * n_alignments, n_cells, n_residue_bytes over those pairs, each once; n_chunks and the times as for a whole fill;
 * pc_last_plan_tasks covers a rows fill too.
 * n_rows == 0: PC_OK, nothing done; n_rows == N is allowed.  PC_ERR_ARG: rows not strictly ascending or out of range, NULL out,
 * bad metric.  PC_ERR_STATE: before upload, on a sharded context (world != 1), aai / peq before pc_upload_residues.
 * PC_ERR_DATA: an empty translation under aai / peq.  pc_fill_rows delivers into host memory; pc_fill_rows_dev leaves the
 * result in HBM (out_dev: device f64[n_rows * N]; stream as for pc_fill_dev).
 */
int pc_fill_rows(pc_ctx* ctx, int metric, int as_distance, const int32_t* rows, int n_rows, double* out_host, pc_stats* stats);
int pc_fill_rows_dev(pc_ctx* ctx, int metric, int as_distance, const int32_t* rows, int n_rows, void* out_dev, void* stream, pc_stats* stats);

/*
 * Groups fill: every within-group pair of a family of groups in one call.  The reference takes the sub-matrix of a group out of
 * the dense matrix (SymMatrix.extract_submatrix, matrix.py:155-167; the pipeline's per-cluster matrices, scripts/phamclust.py:300-317);
 * this call fills the blocks alone: the pairs (s, t), s < t, whose two genomes lie in the same group -- sum of n_c (n_c - 1) / 2
 * pairs instead of N (N - 1) / 2 -- from one upload, with one plan (per chunk) that merges duplicate sequence pairs across ALL groups.
 * members[M]: genome indices, group by group; group_off[n_groups + 1]: group c is members[group_off[c] .. group_off[c + 1]).  Inside
 * a group the members are strictly ascending, so the smaller index is the reference's `source` as in the whole fill (aai is not
 * symmetric); groups may share genomes; a group of 0 or 1 members has no pair.
 * out: the groups' condensed triangles end to end, f64[L]: pair (i, j), i < j, of group c (positions inside the group, n its size)
 * sits at pair_off[c] + i n - i (i + 1) / 2 + (j - i - 1), pair_off[c] = sum over c' < c of n_c' (n_c' - 1) / 2, L = pair_off[n_groups]
 * (scipy's condensed order per group; pc_group_pair_offsets).  All pair indices are 64-bit.  Values are the whole fill's, bit for
 * bit.  The six metrics and PC_AAI_PPOS.  gcs / jc / pocp / af always run on the groups walker: no selector, and pc_last_set_kernel /
 * pc_last_set_launch keep reporting the last whole fill.  aai / peq are cut into successive ranges of row blocks (32 positions) under
 * the rule of pc_set_plan_budget, the 8 bytes per slot of the per-pair count / offset arrays counting against the budget as in a rows
 * fill; same values whatever the cut.  stats: n_pairs = L; n_alignments, n_cells, n_residue_bytes summed over the slots (a pair that
 * sits in two groups counts twice); n_distinct_* per plan; n_chunks and the times as for a rows fill; pc_last_plan_tasks covers a
 * groups fill too.
 * PC_OK, nothing written: n_groups == 0 or L == 0.  PC_ERR_ARG: bad metric; a NULL pointer with L > 0; group_off[0] != 0; group_off
 * decreasing; a member out of range; a group not strictly ascending; M > 2^31-1.  PC_ERR_STATE: before upload, on a sharded context
 * (world != 1), aai / peq before pc_upload_residues.  PC_ERR_DATA: as a whole fill.  pc_fill_groups delivers into host memory;
 * pc_fill_groups_dev leaves the result in HBM (out_dev: device f64[L]; stream as for pc_fill_dev).
 */
int pc_fill_groups(pc_ctx* ctx, int metric, int as_distance, const int32_t* members, const int64_t* group_off, int n_groups,
                   double* out_host, pc_stats* stats);
int pc_fill_groups_dev(pc_ctx* ctx, int metric, int as_distance, const int32_t* members, const int64_t* group_off, int n_groups,
                       void* out_dev, void* stream, pc_stats* stats);
/* Host arithmetic of the groups domain (no GPU; exported for tests, as pc_chunk_plan is).  pc_group_pair_offsets writes pair_off
 * [n_groups + 1] (NULL: nothing) and returns L.  pc_group_tiles lists the live 32 x 32 tiles over the M positions of the groups laid
 * end to end -- (a, b), a <= b: some pair of one group has its first member in block a and its second in block b -- sorted by a,
 * then b, writes at most cap of them (NULL arrays: none) and returns their number T.  Both return PC_ERR_ARG (negative) for
 * group_off[0] != 0 or a decreasing group_off. */
int64_t pc_group_pair_offsets(const int64_t* group_off, int n_groups, int64_t* pair_off);
int64_t pc_group_tiles(const int64_t* group_off, int n_groups, int32_t* tile_row, int32_t* tile_col, int64_t cap);

/*
 * Pair-list fill (PC_VERSION 171): the values of the pairs the caller names, in one call.  This is the reference's most basic interface,
 * METRICS[metric](source, target) (cli.py:30-35, metrics.py:26-253), for a whole list: entry k is the pair with source genome src[k]
 * and target genome tgt[k], and out[k] = METRICS[metric](genomes[src[k]], genomes[tgt[k]], as_distance), in the caller's order.  Every
 * other fill fixes its pair domain by shape (the triangle, whole rows, whole blocks); here the domain is the list: the edges of an
 * adjacency file under another metric, k-nearest lists rescored, a random sample of a collection too large to fill, a spot check.
 * The list is ORIENTED: src[k] is the `source` whatever the index order.  With src[k] < tgt[k] the value is the whole fill's cell, bit
 * for bit; with src[k] > tgt[k] it is the reference's value for the arguments in that order, which differs under aai / aai_ppos / peq
 * where a tie in gene counts makes the source the anchor (metrics.py:208-209) -- no other fill computes that orientation; the four set
 * metrics are symmetric.  src[k] == tgt[k] gives the diagonal, 1.0 - as_distance (matrix.py:467-468).  A pair may be listed any number
 * of times, in either orientation; every entry gets its own value.
 * The library sorts the list on the device by (target, source) and walks blocks of pc_pair_block() = 256 sorted slots, one plan (per
 * chunk) merging the duplicate sequence pairs of everything listed.  The six metrics and PC_AAI_PPOS.  gcs / jc / pocp / af always run
 * on the pairs walker: no selector, and pc_last_set_kernel / pc_last_set_launch keep reporting the last whole fill.  aai / peq are cut
 * into successive ranges of blocks under the rule of pc_set_plan_budget, the 8 bytes per slot of the per-pair count / offset arrays
 * counting against the budget as in a groups fill; same values whatever the cut.  stats: n_pairs = the entries with src != tgt;
 * n_alignments, n_cells, n_residue_bytes summed over the entries (an entry listed twice counts twice); n_distinct_* per plan; n_chunks,
 * n_tasks and the times as for a groups fill (ms_total includes the sort; under gcs / jc / pocp / af ms_plan is the sort and ms_reduce the
 * walker alone); pc_last_plan_tasks covers this call too.
 * The context's state and the metric are checked first, as in every fill; then n_pairs == 0: PC_OK, nothing written.  PC_ERR_ARG, nothing launched and out untouched: bad metric; n_pairs < 0; a NULL pointer with
 * n_pairs > 0; an index outside [0, N) (the message names the entry).  PC_ERR_LIMIT: n_pairs > 2^31-1.  PC_ERR_STATE: before upload, on a
 * sharded context (world != 1), aai / peq before pc_upload_residues.  PC_ERR_DATA: an empty translation under aai / peq, anywhere in
 * the collection, as a whole fill.  pc_fill_pairs delivers into host memory f64[n_pairs]; pc_fill_pairs_dev leaves the result in HBM
 * (out_dev: device f64[n_pairs]; stream as for pc_fill_dev; src and tgt are host memory in both forms, copied before the call returns).
 */
int pc_fill_pairs(pc_ctx* ctx, int metric, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                  double* out_host, pc_stats* stats);
int pc_fill_pairs_dev(pc_ctx* ctx, int metric, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                      void* out_dev, void* stream, pc_stats* stats);
int pc_pair_block(void);     /* slots per block of a pair-list fill (256): host arithmetic, for tests */

/*
 * Joint fill (PC_VERSION 173): up to six metrics of every pair from ONE plan and ONE alignment pass.  peq is
 * round(round(af, 6) * round(aai, 6), 6) (metrics.py:247-253): a peq fill computes af and aai of every pair on its way, and its walk
 * visits every shared pham, which is all that gcs, jc and pocp read.  A caller who wants several metrics of a collection -- why are
 * two genomes far apart under peq: few shared genes (af) or diverged ones (aai)? -- ran the fills one after another, and the aai fill
 * ran the peq fill's alignments again, bit for bit.  Here the reduce walk of the peq fill (k_walk / k_walk_pairs in their joint mode)
 * stores every metric asked for, each finished by the single-metric fill's own expression: every value equals pc_fill's / pc_fill_pairs'
 * of that metric bit for bit, for both as_distance values.
 * metrics: bit m set = metric m of the enum pc_metric is wanted: PC_GCS ... PC_PEQ, bits 0-5.  out[m] must be non-NULL for every set bit; for a
 * clear bit out[m] is not read and nothing behind it is touched.  pc_fill_joint / pc_fill_joint_dev: the whole triangle, every array
 * the condensed f64[N (N - 1) / 2] of pc_fill (host) / pc_fill_dev (HBM; stream as there).  pc_fill_pairs_joint / _dev: the listed
 * pairs under pc_fill_pairs' contract -- oriented, in the caller's order, repeats allowed, src[k] == tgt[k] the diagonal 1.0 -
 * as_distance in every array -- every array f64[n_pairs].  The host forms stage through the context's output buffer, sized for the
 * arrays asked for.
 * The plan is cut into chunks by pc_set_plan_budget's rule exactly as the peq fill's (same chunks; each chunk's walk writes all the
 * arrays for its targets / blocks).  stats are the peq fill's: n_alignments, n_distinct_alignments, n_cells, n_tasks, n_align_launches
 * and n_chunks equal those of pc_fill(PC_PEQ) / pc_fill_pairs(PC_PEQ) on the same context, budget and list; ms_reduce is the joint
 * walk; pc_last_plan_tasks covers these calls too.
 * Refused before anything is launched, the context staying usable -- PC_ERR_STATE: before upload; on a sharded context (world != 1).
 * PC_ERR_ARG: an empty set; a bit above 5 (PC_AAI_PPOS is another alignment pass and no part of this); a set with neither PC_AAI nor
 * PC_PEQ (gcs / jc / pocp / af alone share no alignment pass: four millisecond fills, pc_fill); out NULL, or out[m] NULL for a set
 * bit.  Then the list's checks as pc_fill_pairs makes them (the pair-list forms); PC_ERR_STATE before pc_upload_residues; PC_ERR_DATA:
 * an empty translation, as a peq fill.  No rows, groups, slab, borrow or multi-GPU form.
 */
int pc_fill_joint(pc_ctx* ctx, uint32_t metrics, int as_distance, double* const out_condensed[6], pc_stats* stats);
int pc_fill_joint_dev(pc_ctx* ctx, uint32_t metrics, int as_distance, void* const out_dev[6], void* stream, pc_stats* stats);
int pc_fill_pairs_joint(pc_ctx* ctx, uint32_t metrics, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                        double* const out[6], pc_stats* stats);
int pc_fill_pairs_joint_dev(pc_ctx* ctx, uint32_t metrics, int as_distance, const int32_t* src, const int32_t* tgt, int64_t n_pairs,
                            void* const out_dev[6], void* stream, pc_stats* stats);

/*
 * Edge-list fill: the pairs within a threshold, without the dense matrix.  The reference knows this form of its result twice --
 * matrix_to_adjacency(dist_mat, skip_zero=True) writes it as the pipeline's final file (matrix.py:536-551, scripts/phamclust.py:462-464)
 * and SymMatrix.nearest_neighbors(source, threshold) queries it per node (matrix.py:265-296) -- and derives it from the dense
 * matrix both times.  This call delivers the pairs (s, t), s < t, whose value passes the predicate -- value <= threshold for a
 * distance fill (as_distance != 0), value >= threshold for a similarity fill; a plain f64 compare on the delivered, already
 * round(x, 6) value -- as three parallel arrays src[E], tgt[E], val[E], SORTED BY t, THEN s, in page-locked memory the context
 * owns: valid until the next fill or upload on this context or its destruction (pc_fill_borrow's loan rule).  Values are the
 * whole fill's, bit for bit.  The six metrics and PC_AAI_PPOS.
 * The dense matrix never crosses PCIe and need not fit in HBM: the call fills and compacts successive contiguous ranges of
 * target genomes ("slabs"), one resident at a time, cut by the chunking rule -- pc_chunk_plan over count[t] = t with
 * max_per_chunk = slab_bytes / 8, clamped to 2^31-1 pairs.  slab_bytes = 0: the smallest of the dense triangle, a quarter of the
 * HBM free at the call (the plan of an aai / peq slab takes its own half, pc_set_plan_budget) and the 2^31-1 pair cap.  Each slab
 * is filled as a shard of its targets (every kernel family takes one; same values), then count -> scan -> one 4-byte read-back ->
 * emit -> a copy of exactly that slab's edges.  Consequences: aai / peq merge duplicate sequence pairs per slab only, as a pair
 * shard does per rank; pc_last_set_kernel, pc_last_set_launch and pc_last_plan_tasks describe the LAST slab's fill.  The caller's
 * unsharded state is back in force when the call returns, whatever it returns.
 * stats: summed over the slabs' fills -- n_pairs = N(N-1)/2, n_chunks, the counts and the times added up (the compaction and the
 * copy are not in them: pc_last_edge_times).  *n_slabs: ranges the rule cut (a range holding target 0 alone counts, though it has no pair).
 * PC_OK also for N <= 1 or nothing passing, with *n_edges = 0.  PC_ERR_ARG: bad metric, NaN threshold, negative slab_bytes, a NULL
 * out pointer.  PC_ERR_STATE: before upload, on a sharded context (world != 1: one context walks all the slabs; several GPUs of a
 * node share the walk through pc_multi_fill_edges), aai / peq before pc_upload_residues.  PC_ERR_DATA:
 * as for a whole fill.  Runs on the context's own stream and returns with everything finished.
 */
int pc_fill_edges(pc_ctx* ctx, int metric, int as_distance, double threshold, int64_t slab_bytes,
                  const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook: HIP-event milliseconds of the last pc_fill_edges call that was given stats, summed over its slabs:
 * *ms_compact count + scan + emit, *ms_d2h the copy of the edges to the host; either pointer may be NULL. */
int pc_last_edge_times(const pc_ctx* ctx, float* ms_compact, float* ms_d2h);
/*
 * The edge-list fill under a bar per genome (PC_VERSION 172): pc_fill_edges with the predicate pass(v, bar[s]) || pass(v, bar[t]) in
 * place of pass(v, threshold) -- pass is pc_fill_edges' plain f64 compare, v <= bar on a distance fill, v >= bar on a similarity fill,
 * on the delivered, already round(x, 6) value of the pair (s, t), s < t.  bar: f64[N] in host memory, read during the call only.  It is
 * the candidate pass of a k-nearest search (bar[g] = the worst value genome g still takes): a pair is delivered when either end takes
 * it.  An infinite bar is legal and admits every pair of its genome or none of them on its own account.  With every bar equal to thr
 * the result is pc_fill_edges(thr)'s, element for element.  The walk, the slab cut, the order (t, then s), the loan rule, the values,
 * stats, *n_slabs and pc_last_edge_times are pc_fill_edges'; so are its refusals, with "a NaN bar, naming the genome" and "bar is NULL"
 * (both PC_ERR_ARG, checked where pc_fill_edges checks its threshold) in the NaN threshold's place.  One context; there is no
 * pc_multi_ form and no rows form.
 */
int pc_fill_edges_bars(pc_ctx* ctx, int metric, int as_distance, const double* bar /* f64[N], host */, int64_t slab_bytes,
                       const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);

/*
 * Components fill: the single-linkage clusters at a threshold, without the dense matrix and without an edge list.  labels[g] is
 * the smallest genome index of g's connected component in the graph whose edges are the pairs (s, t) that pass the predicate --
 * pc_fill_edges' (value <= threshold on distances, >= on similarities), or with strict != 0 the strict forms (<, >); a plain f64
 * compare on the delivered, already round(x, 6) value.  With as_distance and strict this is exactly what the reference's
 * hierarchical_clustering(matrix, "single", eps) partitions into (clustering.py:4-51: scikit-learn's distance_threshold is "at or
 * above which clusters will not be merged"), and every "average" / "complete" cluster at eps lies inside one such component.
 * Same walk as pc_fill_edges: the same slab cut (pc_chunk_plan over count[t] = t, slab_bytes / 8 pairs, <= 2^31-1; 0 = automatic),
 * each slab filled as a shard into the resident slab buffer, then ONE pass over it (a lock-free union-find over a parent[N] array
 * that lives on the device across the slabs); after the last slab one labelling pass and one copy of labels[N] plus the 8-byte
 * count.  Nothing is read back per slab.  The labels are canonical: they do not depend on how races between workgroups resolved.
 * *labels points into page-locked memory the context owns (pc_fill_borrow's loan rule: valid until the next fill or upload on this
 * context or its destruction); *n_components = genomes g with labels[g] == g; *n_edges = pairs that passed; *n_slabs and stats as
 * pc_fill_edges gives them (the union and labelling passes are not in stats: pc_last_component_times).
 * PC_OK also for N <= 1 or nothing passing (identity labels).  PC_ERR_ARG: bad metric, NaN threshold, negative slab_bytes, a NULL
 * out pointer.  PC_ERR_STATE: before upload, on a sharded context (world != 1: several GPUs share the walk through
 * pc_multi_fill_components), aai / peq before pc_upload_residues.  On a refusal
 * *labels is NULL and the counts are 0.  The caller's unsharded state is back in force when the call returns, whatever it returns.
 */
int pc_fill_components(pc_ctx* ctx, int metric, int as_distance, double threshold, int strict, int64_t slab_bytes,
                       const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook: HIP-event milliseconds of the last pc_fill_components call that was given stats: *ms_union the union passes
 * summed over its slabs, *ms_labels the labelling pass; either pointer may be NULL. */
int pc_last_component_times(const pc_ctx* ctx, float* ms_union, float* ms_labels);

/*
 * Nearest-neighbours fill: each genome's k closest, without the dense matrix and without a threshold.  The reference answers this per
 * node from its dense matrix -- SymMatrix.nearest_neighbors(source, threshold), matrix.py:265-296: the neighbours closest first,
 * equally close ones in node order.  Let kk = min(k, N - 1).  Row g of nbr[N][kk] and val[N][kk] (row-major) lists the kk genomes
 * h != g that come first in ONE total order: the better value first -- the smaller on a distance fill (as_distance != 0), the larger
 * on a similarity fill; a plain f64 compare on the delivered, already round(x, 6) value of the pair {g, h} -- and among equal values
 * the smaller genome index.  That is nearest_neighbors(g, threshold) with the threshold wide open, cut after kk.  One total order:
 * the result is canonical, it depends neither on the slab cut nor on how any race resolved.  Values are the whole fill's, bit for
 * bit, each pair in the whole fill's orientation.  The six metrics and PC_AAI_PPOS.
 * *nbr and *val point into page-locked memory the context owns (pc_fill_borrow's loan rule: valid until the next fill or upload on
 * this context or its destruction); *k_out = kk; *n_slabs and stats as pc_fill_edges gives them -- the fills' stats summed; the
 * selection passes are not in them: pc_last_nearest_times.
 * Same walk as pc_fill_edges: the same slab cut (pc_chunk_plan over count[t] = t, slab_bytes / 8 pairs, <= 2^31-1; 0 = automatic),
 * each slab filled as a shard into the resident slab buffer, then TWO passes over it -- a slab holds the pairs (s, t), s < t, of its
 * targets, so a genome receives candidates as a target (the row pass) and as a source (the column pass) -- that merge into k slots per
 * genome which live on the device across the slabs; after the last slab one finishing pass and one copy of the N * kk entries.
 * Nothing is read back per slab.  Consequences as for pc_fill_edges: aai / peq merge duplicate sequence pairs per slab only;
 * pc_last_set_kernel, pc_last_set_launch and pc_last_plan_tasks describe the LAST slab's fill.  The caller's unsharded state is back
 * in force when the call returns, whatever it returns.
 * PC_OK also for N <= 1, with *k_out = 0 and nothing written.  PC_ERR_ARG: bad metric, k < 1, negative slab_bytes, a NULL out pointer.
 * PC_ERR_LIMIT: k > PC_NEAREST_MAX_K (a genome's list lives one entry per lane of a wave).  PC_ERR_STATE: before upload, on a sharded
 * context (world != 1: several GPUs share the walk through pc_multi_fill_nearest), aai / peq before pc_upload_residues.  PC_ERR_DATA: as for a whole fill.  On a refusal *nbr and *val are NULL
 * and *k_out is 0.  Runs on the context's own stream and returns with everything finished.
 */
#define PC_NEAREST_MAX_K 64
int pc_fill_nearest(pc_ctx* ctx, int metric, int as_distance, int k, int64_t slab_bytes,
                    const int32_t** nbr, const double** val, int32_t* k_out, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook: HIP-event milliseconds of the last pc_fill_nearest call that was given stats: *ms_select the row and column
 * passes summed over its slabs, *ms_finish the finishing pass; either pointer may be NULL. */
int pc_last_nearest_times(const pc_ctx* ctx, float* ms_select, float* ms_finish);
/*
 * K-nearest lists of a pair list (PC_VERSION 172): what pc_fill_nearest delivers of the whole triangle, of the pairs the caller lists.
 * src / tgt / val: n_pairs entries in host memory, entry e the pair {src[e], tgt[e]} with the value val[e]; in any order and either
 * orientation; the diagonal (src[e] == tgt[e]) is refused, and the caller promises that no pair is listed twice (in either
 * orientation: it would be two candidates).  Every pair is a candidate of BOTH its ends.  Let kk = min(k, N - 1).  count[g] is the
 * number of listed pairs that touch genome g; row g of nbr[N][kk] / val_out[N][kk] (row-major) lists the best min(kk, count[g]) of them
 * -- the other end and the value, bit for bit as given -- in pc_fill_nearest's total order: the better value first (the smaller with
 * as_distance != 0, else the larger; a plain f64 compare), among equal values the smaller genome index.  Slots beyond count[g] hold
 * nbr = -1 and val = NaN.  A list that holds the whole triangle gives pc_fill_nearest's result.
 * *nbr, *val_out and *count point into page-locked memory the context owns (pc_fill_nearest's loan: valid until the next fill, upload
 * or call of this kind on the context, or its destruction); *k_out = kk.  The context supplies N and the work buffers only: neither the
 * sets nor the residues are read, and the shard in force does not matter.  On the device: the 2 n_pairs directed entries (owner << 32 |
 * other, position) are sorted, and one wave per genome selects from its run; no atomics, the result is canonical.
 * PC_OK also for n_pairs == 0 (every count 0, every slot padded) and N <= 1 (*k_out = 0).  In this order -- PC_ERR_STATE: before
 * upload.  PC_ERR_ARG: k < 1.  PC_ERR_LIMIT: k > PC_NEAREST_MAX_K.  PC_ERR_ARG: a NULL out pointer, n_pairs < 0.  PC_ERR_LIMIT:
 * n_pairs > 2^30 (the directed entries number 2 n_pairs and their sort value has 32 bits).  PC_ERR_ARG: src, tgt or val NULL with
 * n_pairs > 0; an entry with an index outside [0, N) or on the diagonal, naming it.  On a refusal *nbr, *val_out and *count are NULL and
 * *k_out is 0; the inputs are never written.  Runs on the context's own stream and returns with everything finished.
 */
int pc_nearest_of_pairs(pc_ctx* ctx, const int32_t* src, const int32_t* tgt, const double* val, int64_t n_pairs, int as_distance, int k,
                        const int32_t** nbr, const double** val_out, const int32_t** count /* i32[N] */, int32_t* k_out);

/*
 * Tree fill: the single-linkage dendrogram, without the dense matrix and without a threshold -- the one delivery form that answers
 * every threshold at once.  The reference computes it from its dense matrix (scipy.cluster.hierarchy.linkage(..., 'single') in
 * _get_tree_order, matrix.py:673-686; AgglomerativeClustering(linkage="single"), clustering.py:4-51).  The dendrogram of single
 * linkage is the minimum spanning tree of the complete graph over the genomes: N - 1 edges, from which the clusters at any
 * threshold (strict or not), the clusters for any cluster count, the linkage matrix and the leaf order follow on the host.
 * ONE total order on the pairs (s, t), s < t: the better value first -- the smaller on a distance fill (as_distance != 0), the larger
 * on a similarity fill; a plain f64 compare on the delivered, already round(x, 6) value -- among equal values the smaller t, then the
 * smaller s (the order of pc_fill_edges' list).  The result is the unique spanning tree Kruskal's algorithm accepts when it takes the
 * pairs in that order: *n_edges = N - 1 edges src[i] < tgt[i] with val[i], delivered ASCENDING in that order -- the merge order of
 * single linkage (on a similarity fill: the maximum spanning tree).  The order is strict, so the tree is canonical: it depends
 * neither on the slab cut, nor on the number of devices, nor on how any race resolved.  Values are the whole fill's, bit for bit,
 * each pair in the whole fill's orientation.  The six metrics and PC_AAI_PPOS.
 * The key.  Every delivered value is k / 10^6 for an integer 0 <= k <= 10^6 (the map is an order-preserving bijection), so the order
 * fits one word: key = micro << 44 | t << 22 | s, micro = k on a distance fill and 10^6 - k on a similarity fill, k = rint(v * 1e6);
 * 20 + 22 + 22 bits, hence PC_TREE_MAX_GENOMES.  ~0 is no key (its value field is above 10^6).  One unsigned 64-bit minimum is the
 * minimum of the total order, and a forest is an array of keys.  pc_tree_key packs a key and pc_tree_key_parts unpacks one (PC_ERR_ARG
 * for a word that is no key: micro > 10^6 or s >= t; host arithmetic, no GPU, exported for tests as pc_chunk_plan is).  The pass over a
 * slab checks what the key relies on -- 0 <= k <= 10^6 and k / 10^6 == v (bit for bit; -0.0 is the millionth 0) -- and counts violations: PC_ERR_DATA.  The count
 * in the message is one of SIGHTINGS, not of values: every Boruvka round scans the slab again and sees only the pairs whose ends lie in
 * different components, so a refused value is counted once per round that met it (at least once, unless its ends were joined before).
 * Same walk as pc_fill_edges: the same slab cut (pc_chunk_plan over count[t] = t, slab_bytes / 8 pairs, <= 2^31-1; 0 = automatic),
 * each slab filled as a shard into the resident slab buffer.  MST(A + B) = MST(MST(A) + B): a forest of at most N - 1 keys stays on
 * the device across the slabs, and per slab Boruvka rounds run over that forest and the slab (ceil(log2 N) rounds are enqueued; a
 * round returns at once when the one before it joined nothing).  Nothing is read back per slab; after the last one the N - 1 keys
 * and the violation count are copied once, sorted and decoded on the host (val = k / 1000000.0).  Consequences as for pc_fill_edges:
 * aai / peq merge duplicate sequence pairs per slab only; pc_last_set_kernel, pc_last_set_launch and pc_last_plan_tasks describe the
 * LAST slab's fill.  The caller's unsharded state is back in force when the call returns, whatever it returns.
 * *src, *tgt and *val point into page-locked memory the context owns (pc_fill_borrow's loan rule); *n_slabs and stats as pc_fill_edges
 * gives them -- the fills' stats summed; the rounds are not in them: pc_last_tree_times.
 * PC_OK also for N <= 1, with *n_edges = 0.  PC_ERR_ARG: bad metric, negative slab_bytes, a NULL out pointer.  PC_ERR_LIMIT: N above
 * PC_TREE_MAX_GENOMES.  PC_ERR_STATE: before upload, on a sharded context (world != 1: several GPUs share the walk through
 * pc_multi_fill_tree), aai / peq before pc_upload_residues.  PC_ERR_DATA: as for a whole fill, and a slab value outside the key's
 * domain.  On a refusal *src, *tgt and *val are NULL and the counts are 0.  Runs on the context's own stream and returns with
 * everything finished.
 */
#define PC_TREE_MAX_GENOMES (1 << 22)
int pc_fill_tree(pc_ctx* ctx, int metric, int as_distance, int64_t slab_bytes,
                 const int32_t** src, const int32_t** tgt, const double** val, int32_t* n_edges, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook, of the last pc_fill_tree call: *ms_rounds the Boruvka rounds summed over its slabs (HIP events; 0 unless the
 * call was given stats), *ms_finish the copy of the keys, their sort and their decoding (host wall clock); either pointer may be NULL. */
int pc_last_tree_times(const pc_ctx* ctx, float* ms_rounds, float* ms_finish);
/* ... *live_rounds the rounds that did work (the round before them joined something, or they were a slab's first) and
 * *launched_rounds the rounds enqueued, both summed over the slabs; live <= launched = slabs with pairs x ceil(log2 N).  Either
 * pointer may be NULL. */
int pc_last_tree_rounds(const pc_ctx* ctx, int32_t* live_rounds, int32_t* launched_rounds);
uint64_t pc_tree_key(int32_t micro, int32_t s, int32_t t);
int pc_tree_key_parts(uint64_t key, int32_t* micro, int32_t* s, int32_t* t);

/*
 * Between-groups fill: for a partition of the N genomes into n_groups groups -- group[g] in [0, n_groups) is genome g's -- the
 * n_groups x n_groups table of the count, sum, minimum and maximum of the pair values between every two groups, and within each group
 * on the diagonal: the minimum is the single-linkage, the maximum the complete-linkage and sum / count the average-linkage distance of
 * two clusters (what the reference's dataset heatmap in cluster order shows, matrix.py / scripts/phamclust.py:433, above its 1,500
 * genome cap); the diagonal holds each group's diameter and mean.  A value enters as its millionths, micro = rint(v * 1e6), of the
 * DISTANCE as filled: every delivered value is round(x, 6), so sum[a][b] is an integer and lo / hi are integers, and the table is
 * exact: it depends neither on the slab cut, nor on the number of devices, nor on the order of any atomic.  The pass checks what that
 * relies on -- 0 <= micro <= 10^6 and micro / 10^6 == v (bit for bit; -0.0 is the millionth 0) -- and counts violations: PC_ERR_DATA; such a value is added
 * nowhere.  as_distance == 0 delivers the SIMILARITY table, which is the distance table inverted -- sum' = count * 10^6 - sum, lo' =
 * 10^6 - hi, hi' = 10^6 - lo, by the fold -- i.e. the table of the matrix SymMatrix.invert() (matrix.py:236-247: round(1 - d, 6), the
 * complement of a millionth) makes of the distance matrix, as every similarity the pipeline writes is made.  It is deliberately not
 * the table of a similarity FILL's values: that fill rounds s where the distance fill rounds 1 - s, and at a decimal tie both round
 * up (one pair in 19,900 under af on the synth200 fixture), so its millionths are not always the complements.
 * Same walk as pc_fill_edges (the slab cut, slab_bytes, 0 = automatic).  Each filled slab goes through ONE pass, k_between_rows: a
 * workgroup takes one target row of the slab, or one segment of pc_between_segment() elements of a long row, accumulates over the
 * sources' groups in a table of n_groups entries in LDS and adds what it touched into one row of the accumulator that stays on the
 * device (sum u64, cnt u64, lo u32, hi u32 per entry).  After the last slab k_between_fold makes the square symmetric, then ONE D2H copy.
 * *sum, *count (int64), *lo, *hi (int32; millionths): [n_groups][n_groups], row-major, symmetric, in page-locked memory the context owns
 * (pc_fill_borrow's loan rule).  An entry no pair fell into -- the diagonal of a one-genome group, every entry of an empty group --
 * reads count = 0, sum = 0, lo = INT32_MAX, hi = -1.  Off the diagonal count[a][b] = n_a n_b, on it n_a (n_a - 1) / 2.  N <= 1: PC_OK,
 * nothing runs on the device, every entry empty.  *n_slabs and stats as pc_fill_edges gives them.
 * PC_ERR_ARG: bad metric, group NULL, n_groups < 1, a label outside [0, n_groups) (the message names the genome), negative slab_bytes,
 * a NULL out pointer.  PC_ERR_LIMIT: n_groups above PC_BETWEEN_MAX_GROUPS (the LDS table of the pass: 16 bytes per group, 32 KB at the
 * limit, four workgroups of 256 threads per compute unit).  PC_ERR_STATE: before upload, on a sharded context (world != 1: several
 * GPUs share the walk through pc_multi_fill_between), aai / peq before pc_upload_residues.  PC_ERR_DATA: as for a whole fill, and a
 * slab value that is no millionth in [0, 1].  On a refusal the four pointers are NULL and *n_slabs is 0.  The caller's unsharded state
 * is back in force when the call returns, whatever it returns.  Runs on the context's own stream and returns with everything finished.
 * The rows form is pc_fill_rows_between, below; this call keeps refusing a label of -1.
 */
#define PC_BETWEEN_MAX_GROUPS 2048
int pc_fill_between(pc_ctx* ctx, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                    const int64_t** sum, const int64_t** count, const int32_t** lo, const int32_t** hi, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook, of the last pc_fill_between or pc_fill_rows_between call: *ms_reduce the passes summed over its slabs, *ms_finish the fold (HIP events; 0
 * unless the call was given stats); either pointer may be NULL. */
int pc_last_between_times(const pc_ctx* ctx, float* ms_reduce, float* ms_finish);
int pc_between_max_groups(void);    /* PC_BETWEEN_MAX_GROUPS */
int pc_between_segment(void);       /* elements of a slab row one workgroup of the pass takes (a longer row is split at multiples of it) */

/*
 * Affinity fill (PC_VERSION 165): how every genome relates to every group of a partition.  group / n_groups, the checks, the millionths
 * and the walk are pc_fill_between's.  For genome g and group b the table holds the sum, minimum and maximum of the millionths of
 * d(g, x) over x in b, x != g; the count is not stored, it is size[b] - [group[g] == b].  The table, N x n_groups entries of 16 bytes
 * (pc_affinity_bytes), stays on the device from the first slab to the last; each filled slab goes through two passes (k_aff_rows:
 * entry [t][group[s]], a workgroup per target row; k_aff_cols: entry [s][group[t]], a wave per block of pc_affinity_block() sources
 * and range of groups), every entry written by exactly one wave per launch, no global atomics on the table.  After the last slab
 * k_aff_finish writes what a caller needs per genome, and ONE D2H copy delivers it:
 *   *own_sum (int64), *own_lo, *own_hi (int32): [N], the genome's entry for its own group (a medoid is the member with the smallest
 *       own_sum; own_sum / (size - 1) is the a of a silhouette)
 *   *near_group (int32): [3][N], the OTHER non-empty group that is nearest by 0: the smallest mean (sum_b * size_c against sum_c * size_b
 *       in 64-bit integers), 1: the smallest minimum, 2: the smallest maximum; ties go to the smaller group index; -1 where no other
 *       non-empty group exists
 *   *near_sum (int64), *near_lo, *near_hi (int32): [N], the value that made it nearest -- the sum of group near_group[0][g], the minimum
 *       of group near_group[1][g], the maximum of group near_group[2][g]; 0 / INT32_MAX / -1 where there is none
 *   *tab_sum (int64), *tab_lo, *tab_hi (int32): with want_table != 0 the whole table, [N][n_groups] row-major; else NULL
 * An entry no pair falls into reads sum 0, lo INT32_MAX, hi -1.  as_distance == 0 delivers the statement of the inverted matrix (see
 * pc_fill_between): the nearest groups are chosen on the distances and are the same, every reported value is complemented -- sum' =
 * count * 10^6 - sum, table and own entries lo' = 10^6 - hi, hi' = 10^6 - lo, near_lo' = 10^6 - near_lo, near_hi' = 10^6 - near_hi.
 * All arrays lie in page-locked memory the context owns (pc_fill_borrow's loan rule).  N <= 1: PC_OK, nothing runs on the device.
 * The two passes each see every element of a slab and each leave a value that is no millionth in [0, 1] out; the row pass alone counts
 * it, so the count in the PC_ERR_DATA message is the number of such values, as pc_fill_between's is.
 * Refusals as pc_fill_between's, and PC_ERR_LIMIT when the table (with want_table: and its converted copy) takes more than half of the
 * HBM that is free when the call begins; the message carries both numbers.  The rows form is pc_fill_rows_affinity, below; this call
 * keeps refusing a label of -1.
 */
int pc_fill_affinity(pc_ctx* ctx, int metric, int as_distance, const int32_t* group, int n_groups, int want_table, int64_t slab_bytes,
                     const int64_t** own_sum, const int32_t** own_lo, const int32_t** own_hi, const int32_t** near_group,
                     const int64_t** near_sum, const int32_t** near_lo, const int32_t** near_hi,
                     const int64_t** tab_sum, const int32_t** tab_lo, const int32_t** tab_hi, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook, of the last pc_fill_affinity or pc_fill_rows_affinity call: the row passes and the column passes summed over its slabs, and the finish (HIP
 * events; 0 unless the call was given stats); any pointer may be NULL. */
int pc_last_affinity_times(const pc_ctx* ctx, float* ms_rows, float* ms_cols, float* ms_finish);
int pc_affinity_block(void);        /* consecutive sources one wave of the column pass takes */
int64_t pc_affinity_bytes(int64_t n, int64_t n_groups);   /* the resident table: 16 n n_groups + 8; -1: not representable */
/* Test hook, host arithmetic (PC_VERSION 166): the column pass's cut of the groups into ranges, as the fill makes it from the device's
 * compute-unit count (want = ceil(16 n_cu / ceil(N / pc_affinity_block()))).  goff[n_groups + 1]: each group's run among the genomes
 * sorted by (group, index), goff[0] = 0 ascending to goff[n_groups] = N.  Writes the range starts followed by n_groups into
 * bounds_out[cap] and returns the number of ranges R <= max(1, min(n_groups, want)): R + 1 bounds, strictly ascending (no range is
 * empty of groups).  cap == 0: only the count.  PC_ERR_ARG: a NULL pointer, n_groups < 1, goff that is no such array, cap too small. */
int pc_affinity_ranges(const int32_t* goff, int n_groups, int n, int want, int32_t* bounds_out, int cap);

/*
 * The rows forms of the edge-list, components and tree fills: a STORED result grown by new genomes.  rows[n_rows] are the query genomes
 * -- the new ones -- under pc_fill_rows' contract (strictly ascending indices of the uploaded collection, which holds old and new
 * genomes in fill order); the pairs of the call are those that touch a query genome, each once (a pair of two query genomes in the row
 * of the smaller): n_rows * (N - 1) - n_rows (n_rows - 1) / 2 pairs instead of N (N - 1) / 2.  What is stored stands for the pairs
 * among the other genomes.  It can, exactly: the old genomes keep their relative order inside the grown collection, so the map from
 * old to new indices is strictly increasing and every comparison the fills make among old pairs (value, then target, then source) is
 * unchanged under it -- the stored result, re-indexed by the caller, is what a fill of the old block would deliver in the new indexing.
 * Every index in these calls, seeds included, is in the UPLOADED collection's numbering.
 * The walk: the query rows are cut into consecutive ranges of at most max(1, slab_bytes / 8 / N) rows (slab_bytes == 0: automatic, by
 * the free HBM as pc_fill_edges decides it); each range is filled by the rows fill itself into the resident slab buffer as f64[m][N]
 * and goes through the rows form of the fill's pass (the same predicate, ballot ranking, union and key as the triangular pass; the
 * diagonal and the second copy of a pair of two query genomes are skipped).  *n_slabs = the ranges walked.  Values are the whole
 * fill's, bit for bit, each pair in the whole fill's orientation.  One GPU; the six metrics and PC_AAI_PPOS.
 *   pc_fill_rows_edges       the passing pairs of the call (threshold as pc_fill_edges), sorted by target, then source (one host sort:
 *                            the passes emit row-major); at most n_rows * N.  The grown list is the stored list re-indexed, merged
 *                            with this one by (target, source): the caller's part (matrix.edges_extend).
 *   pc_fill_rows_components  seed_labels (i32[N], or NULL: every genome its own component) is the initial parent[]: the stored labelling
 *                            re-indexed, a new genome labelling itself.  0 <= seed_labels[g] <= g and seed_labels[seed_labels[g]] ==
 *                            seed_labels[g], else PC_ERR_ARG.  The passing pairs of the call are united into it (predicate and strict as
 *                            pc_fill_components): *labels the grown collection's canonical labels; *n_edges counts the call's passing
 *                            pairs only.
 *   pc_fill_rows_tree        the n_seed seed edges (the stored tree re-indexed; a forest) are packed with pc_tree_key -- a seed that is
 *                            no key (source < target < N, a value that is a millionth in [0, 1]) or n_seed > N - 1: PC_ERR_ARG -- and
 *                            are the resident forest in place of the empty one: MST(A + B) = MST(MST(A) + B) with A the pairs among
 *                            old genomes, B the call's.  The result has N - 1 edges iff seeds and the call's pairs connect the
 *                            collection; otherwise PC_ERR_HIP ("the forest holds ... edges").
 * n_rows == 0 is PC_OK: with seeds the seeds' labelling or tree, without them every genome its own component (and, N > 1, no tree).
 * Outputs, loans, stats and the refusals' order are the triangular calls' (before upload, sharded context, PC_TREE_MAX_GENOMES, a NULL
 * out pointer, a NaN threshold, negative slab_bytes, missing residues); then rows (pc_fill_rows' PC_ERR_ARG), then the seeds.
 * pc_last_edge_times / pc_last_component_times / pc_last_tree_times / pc_last_tree_rounds report on these calls too (the edges' host
 * sort is added to ms_d2h).  Not built: several GPUs.
 */
int pc_fill_rows_edges(pc_ctx* ctx, int metric, int as_distance, double threshold, const int32_t* rows, int n_rows, int64_t slab_bytes,
                       const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);
int pc_fill_rows_components(pc_ctx* ctx, int metric, int as_distance, double threshold, int strict, const int32_t* rows, int n_rows,
                            const int32_t* seed_labels /* i32[N] or NULL */, int64_t slab_bytes,
                            const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);
int pc_fill_rows_tree(pc_ctx* ctx, int metric, int as_distance, const int32_t* rows, int n_rows,
                      const int32_t* seed_src, const int32_t* seed_tgt, const double* seed_val, int32_t n_seed, int64_t slab_bytes,
                      const int32_t** src, const int32_t** tgt, const double** val, int32_t* n_edges, int32_t* n_slabs, pc_stats* stats);
/* Test hook, host arithmetic: the values one workgroup of a rows pass covers (pass_kind 0: edge count / emit, 1: union, 2: tree scan;
 * anything else: 0) -- what a test of the passes' workgroup seams sizes its slabs by. */
int pc_rows_pass_span(int pass_kind);

/*
 * The rows form of the nearest-neighbours fill: stored k-nearest lists grown by new genomes (PC_VERSION 163).  rows, the walk, the
 * values and the index space as above.  seed_nbr / seed_val [N][k_seed], row-major in the UPLOADED collection's numbering, are the stored
 * lists re-indexed: row g of an old genome its best old neighbours, best first; rows of query genomes are ignored.  With N_old = N -
 * n_rows and kk = min(k, N - 1): k_seed >= min(kk, N_old - 1), else PC_ERR_ARG (a shorter stored list cannot decide kk neighbours);
 * columns beyond kk (and beyond N_old - 1) are cut; NULL seeds only while N_old <= 1.  A seed entry that is out of range, names a query genome or the genome
 * itself, or a row that does not ascend in (value, better first; then index): PC_ERR_ARG.  All refusals come before anything is launched,
 * with the outputs nulled, and leave the context usable.  The stored lists replace the empty ones on the device; each slab of query rows
 * goes through two passes (k_nn_qrows: a query genome's list from its row, every genome but itself a candidate; k_nn_qcols: the slab's
 * rows as candidates of the old genomes' lists).  Exact: every old candidate outside a stored list is worse, in the total order, than
 * every entry in it, so the best kk of {stored list} + {pairs with the new genomes} is the best kk of all N - 1.  *nbr / *val [N][*k_out]
 * as pc_fill_nearest delivers them, equal to its result over the whole collection.  n_rows == 0: the seed re-laid to kk columns; n_rows
 * == N: pc_fill_nearest; N <= 1 as there.  Refusals' order: pc_fill_nearest's, then rows, then the seed.  pc_last_nearest_times reports
 * on this call too.  One GPU.
 */
int pc_fill_rows_nearest(pc_ctx* ctx, int metric, int as_distance, int k, const int32_t* rows, int n_rows,
                         const int32_t* seed_nbr, const double* seed_val, int32_t k_seed, int64_t slab_bytes,
                         const int32_t** nbr, const double** val, int32_t* k_out, int32_t* n_slabs, pc_stats* stats);
/* Test hook, host arithmetic: the tile edge of that call's column pass (rows and columns of the slab a workgroup stages at a time). */
int pc_nearest_rows_tile(void);

/*
 * The rows form of the affinity fill (PC_VERSION 168): new genomes placed against stored clusters.  rows[n_rows] -- pc_fill_rows' contract,
 * the rows walk and its slabs (f64[m][N], slab_bytes) as above -- are the QUERY genomes; group[N] / n_groups is the partition, and here,
 * and only here, group[g] may be -1: a member of no group (a new genome not yet placed).  Values enter as millionths of the DISTANCE
 * under pc_fill_affinity's rule; as_distance == 0 complements every reported value by its formulas; the nearest groups are chosen on
 * distances.  The definition everything is held to:
 *   Row table.  Query k is q = rows[k].  Entry [k][b] holds the sum, minimum and maximum of the millionths of d(q, x) over all x != q
 *       with group[x] == b -- x may itself be a query.  Its count is not stored: size[b] - [group[q] == b], size[b] the genomes
 *       labelled b, queries included.  An entry no pair falls into reads 0 / INT32_MAX / -1.
 *   Per query, [n_rows], as pc_fill_affinity states it per genome: *own_sum / *own_lo / *own_hi (empty when group[q] == -1);
 *       *near_group [3][n_rows], the nearest group b != group[q] with a non-zero count by the smallest mean (64-bit integers), minimum
 *       and maximum, ties to the smaller index, -1: none -- an unlabelled query has no own group, so every non-empty group is a
 *       candidate; *near_sum / *near_lo / *near_hi; with want_table *tab_sum / *tab_lo / *tab_hi [n_rows][n_groups], else NULL.
 *   Own-group gain, with want_gain, [N] (else NULL): for a genome g that is NOT a query and has group[g] >= 0, the sum, minimum and
 *       maximum of the millionths of d(g, x) over the query genomes x with group[x] == group[g]; empty for a query, for an unlabelled
 *       genome and where no such x exists.  It is what the queries add to g's own entry: with own_old from an affinity fill of the
 *       collection without the queries, own_old (+) gain -- sums added, the smaller lo, the larger hi -- is own of pc_fill_affinity
 *       over the whole collection, so stored own sums, the medoids and the a-term of every silhouette grow exactly.  (as_distance ==
 *       0: complemented over its count, the queries labelled group[g].)  The nearest-other-group columns of OLD genomes cannot grow
 *       without the stored N x n_groups table: not built.
 * Consequence: with every genome labelled, query k's row and per-query outputs equal entry rows[k] of pc_fill_affinity's on the same
 * group, integer for integer, for any subset of rows and any slab cut.
 * On the device: n_rows x n_groups entries and the gain's N, 16 bytes each, stay resident (refused with PC_ERR_LIMIT above half of the
 * free HBM, with want_table counting the table's converted copy); each slab of query rows goes through k_aff_qrows (a workgroup per
 * query row; a query's row lies in one slab and is written once) and, with want_gain, k_aff_qcols (a lane per column, one writer per
 * genome and launch); after the last slab k_aff_qfinish and ONE D2H copy.  Every entry has one writer per launch; no global atomics
 * but the violation count.  A value that is no millionth in [0, 1] is left out and counted once per PAIR (a pair of two labelled
 * queries stands in two rows: the row of the smaller counts it); columns of unlabelled genomes and the diagonal are never read.
 * PC_ERR_DATA carries the count.
 * All arrays lie in page-locked memory the context owns (pc_fill_borrow's loan rule).  n_rows == 0 and N <= 1: PC_OK, nothing runs on
 * the device, every entry empty; n_rows == N is allowed.  Refusals in pc_fill_affinity's order -- the label check admits -1 and names
 * the genome otherwise -- then rows (pc_fill_rows' PC_ERR_ARG); all before anything is launched, with the outputs nulled, and the
 * context stays usable.  One GPU: a sharded context is refused (PC_ERR_STATE).  pc_last_affinity_times reports on this call too (rows:
 * k_aff_qrows, cols: k_aff_qcols).
 */
int pc_fill_rows_affinity(pc_ctx* ctx, int metric, int as_distance, const int32_t* group, int n_groups, const int32_t* rows, int n_rows,
                          int want_table, int want_gain, int64_t slab_bytes,
                          const int64_t** own_sum, const int32_t** own_lo, const int32_t** own_hi, const int32_t** near_group,
                          const int64_t** near_sum, const int32_t** near_lo, const int32_t** near_hi,
                          const int64_t** tab_sum, const int32_t** tab_lo, const int32_t** tab_hi,
                          const int64_t** gain_sum, const int32_t** gain_lo, const int32_t** gain_hi, int32_t* n_slabs, pc_stats* stats);

/*
 * The rows form of the between-groups fill (PC_VERSION 169): a stored table grown by new genomes.  rows[n_rows] -- pc_fill_rows'
 * contract, the rows walk and its slabs (f64[m][N], slab_bytes) as above -- are the QUERY genomes (the new ones); group[N] / n_groups
 * is the partition of the grown collection, and group[g] may be -1, for a query or an old genome: a member of no group, in no pair of
 * the table.  The pairs of the call are those with a query genome at one end and both ends labelled; a pair of two queries is taken
 * once.  Values enter as millionths of the DISTANCE under pc_fill_between's rule, as_distance == 0 inverts in the fold.
 *   The seed: seed_sum / seed_count (int64) and seed_lo / seed_hi (int32), [n_groups][n_groups] in the result layout and IN THE CALL'S
 *       DIRECTION -- what pc_fill_between delivers for the same labels over the genomes that are no query rows; all four NULL: no seed.
 *       Counts and sums add, minima and maxima only move outward, everything is an integer: seed (+) the pairs of the call IS the
 *       table of the grown collection.  The seed is checked on the host before any GPU work, PC_ERR_ARG naming the entry: not
 *       symmetric; emptiness inconsistent (count 0 goes with sum 0, lo INT32_MAX, hi -1, and a full entry has none of those); lo > hi or
 *       either outside [0, 10^6]; sum outside [count lo, count hi]; a count that is not the partition's own -- with old[b] the genomes
 *       labelled b that are no query rows, count[a][b] must be old[a] old[b], and old[a] (old[a] - 1) / 2 on the diagonal: every pair
 *       of a fill is counted, so a table of another partition or genome set fails here.  Some but not all of the four: PC_ERR_ARG.
 * Contract: (a) every genome labelled and the seed pc_fill_between's over the non-query genomes with the same labels -> the result is
 * pc_fill_between over the whole collection, integer for integer, for any slab cut and both directions; (b) no seed and rows = all
 * genomes -> pc_fill_between itself; (c) no seed -> the table over exactly the pairs with at least one labelled query end and both
 * ends labelled.
 * On the device: the seed, complemented to distances where as_distance == 0, replaces the empty accumulator (entries a <= b; the fold
 * adds the two orientations); each slab of query rows goes through ONE pass, k_between_qrows -- grid (rows of the slab, segments of
 * pc_between_segment() elements of a row), a workgroup per segment of one row, the same LDS table, wave reduction and relaxed
 * agent-scope atomics without a return value as k_between_rows; the value of an element that is no pair of the call (the diagonal, the
 * second copy of a pair of two queries, a column of an unlabelled genome, the row of an unlabelled query) is never looked at, so a
 * refused value is counted once per PAIR (PC_ERR_DATA carries the count) -- then k_between_fold as it is and ONE D2H copy.
 * Outputs, *n_slabs, stats and pc_last_between_times as pc_fill_between's.  n_rows == 0: the seed comes back unchanged (without one:
 * every entry empty).  N <= 1: every entry empty, and a seed must be all empty.  n_rows == N is allowed.  Refusals in
 * pc_fill_between's order -- the label check admits -1 -- then rows (pc_fill_rows' PC_ERR_ARG), then the seed; all before anything
 * is launched, with the outputs nulled, and the context stays usable.  One GPU: a sharded context is refused (PC_ERR_STATE); there is
 * no pc_multi_* form, n_groups stays within PC_BETWEEN_MAX_GROUPS, and genomes cannot be REMOVED from a stored table (a minimum cannot
 * be un-taken).
 */
int pc_fill_rows_between(pc_ctx* ctx, int metric, int as_distance, const int32_t* group, int n_groups, const int32_t* rows, int n_rows,
                         const int64_t* seed_sum, const int64_t* seed_count, const int32_t* seed_lo, const int32_t* seed_hi, int64_t slab_bytes,
                         const int64_t** sum, const int64_t** count, const int32_t** lo, const int32_t** hi, int32_t* n_slabs, pc_stats* stats);

/*
 * Distribution fill (PC_VERSION 170): the exact histogram of every pair value of the collection, without the dense matrix.  A delivered
 * value is round(x, 6), one of the pc_hist_bins() = 10^6 + 1 millionths in [0, 1] (checked per value under pc_fill_between's rule: -0.0
 * is the millionth 0, anything else that is no millionth in [0, 1] is counted and enters no bin), so the whole distribution is one
 * integer array, 8 MB whatever N is.  From it follow, exactly and for every threshold at once: the count of pairs within a threshold
 * (pc_fill_edges' *n_edges), every quantile, minimum and maximum, mean, variance and skewness.
 *   group / n_groups   NULL: one class.  int32[N], every label in [0, n_groups) (no cap on n_groups: labels are only compared): two
 *                      classes, class 0 the pairs whose genomes share a label ("within"), class 1 the others ("between").
 *   *hist              int64[*n_classes][pc_hist_bins()], the context's pinned memory, lent under pc_fill_borrow's rule; bin k of a class
 *                      counts its pairs of millionth k.  *n_pairs is the sum of all bins, N (N - 1) / 2; with a partition class 0 sums
 *                      to the sum over the groups of n_c (n_c - 1) / 2.
 * The slabs are always filled as DISTANCES; as_distance == 0 delivers the histogram of the inverted matrix, every class reversed (bin k
 * <-> 10^6 - k), as pc_fill_between inverts its table -- deliberately not the histogram of a similarity fill's values (at a decimal tie
 * 1 - d and d both round up).
 * Same walk as pc_fill_edges (the slab cut, slab_bytes, 0 = automatic).  Each filled slab goes through ONE pass, k_hist_pass: a workgroup
 * takes a chunk of 4,096 elements and counts the keys class << 20 | millionth in an open-addressing table in LDS -- pc_hist_table_slots()
 * slots; the first slot of a key is (key * 2654435761 mod 2^32) >> (32 - log2 slots), then linear probing over at most pc_hist_probes()
 * slots; an insert that finds them all held by other keys adds to the global bin directly -- after the wave's most frequent keys were
 * added by one lane each; at the end of the chunk every occupied slot is ONE relaxed agent-scope 64-bit add into the resident state,
 * u64[classes][bins] and the violation count, which stays on the device from the first slab to the last.  After the last slab
 * k_hist_finish (the reversal), then ONE D2H copy.  The moments are the caller's: it has the whole array.
 * Refusals in pc_fill_between's order and wording (without its cap on n_groups); PC_ERR_DATA: values that are no millionth in [0, 1],
 * with their count; the context stays usable.  N <= 1: PC_OK, nothing runs on the device, every bin zero.
 */
int pc_fill_hist(pc_ctx* ctx, int metric, int as_distance, const int32_t* group /* i32[N] or NULL */, int n_groups, int64_t slab_bytes,
                 const int64_t** hist, int32_t* n_classes, int64_t* n_pairs, int32_t* n_slabs, pc_stats* stats);
/* Test / tuning hook, of the last pc_fill_hist or pc_fill_rows_hist call: *ms_pass the passes summed over its slabs, *ms_finish the finish (HIP events; 0
 * without stats). */
int pc_last_hist_times(const pc_ctx* ctx, float* ms_pass, float* ms_finish);
int pc_hist_bins(void);             /* 1000001 */
int pc_hist_table_slots(void);      /* slots of the pass's LDS table (a power of two) */
int pc_hist_probes(void);           /* slots an insert tries before it adds to the global bin */
/*
 * The rows form of the distribution fill (PC_VERSION 170): a stored histogram grown by new genomes.  rows[n_rows] -- pc_fill_rows'
 * contract -- are the query genomes; the pairs of the call are those that touch one, each once (a pair of two queries in the smaller
 * one's row; the diagonal and the second copy are never looked at: neither counted nor refused).  seed_hist, int64[n_classes][bins] in the
 * call's DIRECTION or NULL, is what pc_fill_hist delivers for the same labels over the genomes that are no query rows; the result is seed
 * + rows, which is pc_fill_hist over the whole collection, bin for bin, for any slab cut and both directions.  Refused (PC_ERR_ARG): a
 * seed with a negative bin, a seed whose total is not N_old (N_old - 1) / 2, with a partition a seed whose class 0 is not the old
 * genomes' within count -- necessary checks, not sufficient ones: a histogram cannot name its pairs.  A label of -1 is refused here too.
 * Refusals in pc_fill_hist's order, then rows, then the seed.  One GPU: a sharded context is refused; there is no pc_multi_* form.
 */
int pc_fill_rows_hist(pc_ctx* ctx, int metric, int as_distance, const int32_t* group, int n_groups, const int32_t* rows, int n_rows,
                      const int64_t* seed_hist /* i64[n_classes][bins] or NULL */, int64_t slab_bytes,
                      const int64_t** hist, int32_t* n_classes, int64_t* n_pairs, int32_t* n_slabs, pc_stats* stats);

/* Root only: permute `world` gathered shards (f64[world * pc_shard_stride()], device)
 * into scipy condensed order (device f64[N(N-1)/2]). */
int pc_assemble_dev(pc_ctx* ctx, const void* gathered_dev, int world, void* out_condensed_dev, void* stream);

/*
 * Alignment-sliced multi-GPU route for aai / peq (replaces, like pc_fill_shard_dev + the gather, the joblib fan-out of
 * matrix.py:432-497 -- but splits the ALIGNMENTS, not the genome pairs): every rank holds the same upload, unsharded, and
 *   1. pc_plan_dev        plans the whole fill (identical on every rank; stats->n_distinct_alignments = length of `res`),
 *   2. pc_align_slice_dev aligns every slice_world-th task of each launch class starting at slice_rank and writes
 *                         (n_ident, aln_len) pairs -- 8 bytes per distinct alignment -- into res_dev, zeros elsewhere,
 *   3. the caller sums the ranks' res arrays onto the root (one reduce; as 64-bit integers: exactly one rank contributes
 *      a non-zero entry), and
 *   4. pc_reduce_dev      on the root turns the summed res into the condensed matrix.
 * Every distinct (row sequence, column sequence) pair is aligned once per JOB (the pair-sharded route merges duplicates
 * per rank only) and the ranks' work is equal by construction.  The plan stays valid until the next upload, shard change
 * or fill on the context.  metric: PC_AAI, PC_PEQ or PC_AAI_PPOS.
 */
int pc_plan_dev(pc_ctx* ctx, int metric, void* stream, pc_stats* stats);
int pc_align_slice_dev(pc_ctx* ctx, int slice_rank, int slice_world, void* res_dev, void* stream, pc_stats* stats);
int pc_reduce_dev(pc_ctx* ctx, int metric, int as_distance, const void* res_dev, void* out_condensed_dev, void* stream);

/*
 * One process, several GPUs -- what SURVEY 8(b) specified as pc_ctx_create(out, device_ids, n_dev): the reference spreads the pair
 * list over `cpus` worker processes inside matrix_de_novo (matrix.py:471-493); this spreads it over the GPUs of the node from ONE
 * process, the library owning a context per device and a host thread per device for the length of each call.  Same static shard as
 * the one-process-per-GPU route above (the cost-balanced deal of the target genomes), same single exchange -- every device copies
 * its shard into the root's gather buffer, device to device (peer copies over xGMI) -- same device-side assembly; nothing to launch,
 * no interpreter, framework import or process group per GPU (those cost ~2.5 s per job: profiles/r04/final/launch_cost.txt).
 * device_ids[0] is the root (it delivers the matrix); an id may repeat (several contexts on one GPU: how the tests rehearse this on
 * a one-GPU box).  One host thread calls in.
 *   pc_multi_upload(m, g, with_residues)  every device, in parallel; with_residues = 0: what the four set metrics need
 *   pc_multi_upload_residues(m, g)        what aai / peq need on top (g: the same packed genomes)
 *   pc_multi_fill_borrow(...)             the whole matrix: *out_host -> f64[N(N-1)/2], scipy condensed order, in page-locked memory
 *                                         of the root context, valid until the next fill or upload; stats: NULL or an array of
 *                                         pc_multi_devices(m) entries (each device's own fill); exchange_ms / assemble_ms: NULL or
 *                                         the slowest device's copy to the root / the root's permutation (HIP events)
 */
typedef struct pc_multi pc_multi;
int pc_multi_create(pc_multi** out, const int* device_ids, int n_dev);
void pc_multi_destroy(pc_multi* m);
int pc_multi_devices(const pc_multi* m);
/* How each device's shard will reach the root, decided in pc_multi_create and never hidden: granted[r] (pc_multi_devices() entries,
 * may be NULL) = one of the values below.  Returns the number of devices whose copies are NOT device to device (the runtime stages
 * them through host memory: correct, slower) and leaves their reasons -- the runtime's own error text, one line per device -- for
 * pc_last_error(); 0 when every copy is a peer copy or stays on the root's device.  The reference has no counterpart: its workers
 * return results through joblib's pickling (matrix.py:488-491). */
typedef enum {
    PC_PEER_SAME_DEVICE = 2,    /* the root itself, or another context on the root's GPU (rehearsal): device-to-device copy */
    PC_PEER_ENABLED = 1,        /* hipDeviceEnablePeerAccess granted (or was already on): hipMemcpyPeerAsync over xGMI     */
    PC_PEER_UNAVAILABLE = 0,    /* hipDeviceCanAccessPeer says no                                                         */
    PC_PEER_FAILED = -1         /* the query or the enable call returned an error                                          */
} pc_peer_access;
int pc_multi_peer_access(const pc_multi* m, int32_t* granted);
int pc_multi_upload(pc_multi* m, const pc_packed* genomes, int with_residues);
int pc_multi_upload_residues(pc_multi* m, const pc_packed* genomes);
int pc_multi_set_tie_rule(pc_multi* m, int rule);
int pc_multi_fill_borrow(pc_multi* m, int metric, int as_distance, const double** out_host, pc_stats* stats, float* exchange_ms, float* assemble_ms);

/*
 * The three fills that deliver a result without the dense matrix, over the devices of `m`: pc_multi_fill_edges, _components and
 * _nearest.  Each has the contract of its single-context namesake (pc_fill_edges, pc_fill_components, pc_fill_nearest) word for word
 * -- values, order, canonical result, PC_OK for N <= 1, PC_ERR_ARG / LIMIT / STATE / DATA, output pointers nulled on a refusal --
 * and its result does not depend on the number of devices.  Results live in page-locked memory of the ROOT context under the loan
 * rule (valid until the next fill or upload on `m`).  stats: NULL or an array of pc_multi_devices(m) entries, each device's summed
 * fills (a device whose stretch is empty reports zeros); *n_slabs: the sum over the devices.  One device (world == 1): the
 * single-context call.  Every context is unsharded when a call returns, whatever it returns; pc_multi_fill_borrow deals anew on every
 * call, so the two kinds of fill do not disturb each other.  PC_ERR_STATE: before pc_multi_upload; aai / peq before the residues.
 * The deal.  The slab walk needs consecutive targets, so the pair shard's scattered deal cannot serve: device r walks ONE contiguous
 * stretch [bounds[r], bounds[r + 1]) of targets and cuts it into slabs by the single-context rule -- pc_chunk_plan over count[t] = t
 * for the targets of the stretch, so its first range starts at bounds[r].  The root computes the bounds once per call:
 * pc_stretch_plan over cost[t] = target_cost[t] + 2000 t for aai / peq (pc_set_shard_balanced's formula; target_cost the DP cells per
 * target of its COUNT walk, computed on the root without leaving a deal in force), cost[t] = t for gcs / jc / pocp / af.  aai / peq
 * merge duplicate sequence pairs per slab only, so target_cost overstates a stretch's work unevenly: the deal balances what it can
 * count (profiles/multi_slab_fill.txt states the imbalance it leaves).  pc_multi_last_stretches: the bounds of the last such call.
 * What travels.  Every device runs its stretch with the call's state on ITS device; then, once:
 *   nearest     key[N][kk] and nbr[N][kk], 12 N kk bytes per device, into a staging slice on the root (hipMemcpyPeerAsync, or a
 *               device-to-device copy on the root's own GPU); ONE launch of k_nn_merge (one wave per genome) merges them, in key space,
 *               into the root's lists before its finishing pass: the result is the K smallest of one total order, so lists merge by it
 *   components  parent[N], 4 N bytes per device, and its 8-byte count of passing pairs (summed on the host: a pair lies in exactly one
 *               stretch); ONE launch of k_cc_merge unites every genome with its parent in each foreign forest, then the root labels
 *   edges       no kernel: the devices' counts are known after their walks, the root's pinned arrays are grown to the total and each
 *               device's edges copied behind those of the ranks before it -- stretches ascend in targets and each list is sorted by
 *               (t, s), so the concatenation is
 * Devices with an empty stretch (more devices than targets with pairs) launch nothing and ship nothing.
 * pc_multi_last_slab_times: of the last such call, *ms_exchange the slowest device's copy to the root (HIP events; edges: the host
 * copy into the root's arrays, wall clock) and *ms_merge the root's merge kernel (edges: 0); either pointer may be NULL.
 */
int pc_multi_fill_edges(pc_multi* m, int metric, int as_distance, double threshold, int64_t slab_bytes,
                        const int32_t** src, const int32_t** tgt, const double** val, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);
int pc_multi_fill_components(pc_multi* m, int metric, int as_distance, double threshold, int strict, int64_t slab_bytes,
                             const int32_t** labels, int32_t* n_components, int64_t* n_edges, int32_t* n_slabs, pc_stats* stats);
int pc_multi_fill_nearest(pc_multi* m, int metric, int as_distance, int k, int64_t slab_bytes,
                          const int32_t** nbr, const double** val, int32_t* k_out, int32_t* n_slabs, pc_stats* stats);
/* pc_fill_tree over the devices of `m`, on the same terms and with the same deal.  MST(A + B) = MST(MST(A) + MST(B)): every device
 * builds the forest of its stretch and ships its keys and their count once, 8 N + 16 bytes, into a staging slice on the root; the root
 * runs Boruvka rounds over its own forest and the staged ones (lists of keys only, no slab), then finishes as the single-context call
 * does.  pc_multi_last_slab_times: the slowest device's copy and the root's merge rounds. */
int pc_multi_fill_tree(pc_multi* m, int metric, int as_distance, int64_t slab_bytes,
                       const int32_t** src, const int32_t** tgt, const double** val, int32_t* n_edges, int32_t* n_slabs, pc_stats* stats);
/* pc_fill_between over the devices of `m`, on the same terms and with the same deal.  Every device accumulates over its stretch of
 * targets and ships its raw accumulator once, 24 n_groups^2 + 8 bytes, into a staging slice on the root; ONE launch of k_between_merge
 * adds sums and counts and takes the extremes (a pair lies in exactly one stretch: nothing is counted twice), then the root folds as
 * the single-context call does.  pc_multi_last_slab_times: the slowest device's copy and the root's merge. */
int pc_multi_fill_between(pc_multi* m, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                          const int64_t** sum, const int64_t** count, const int32_t** lo, const int32_t** hi, int32_t* n_slabs, pc_stats* stats);
/* pc_fill_affinity over the devices of `m`, on the same terms and with the same deal.  Every device fills its table over its stretch of
 * targets and ships it once, 16 N n_groups + 8 bytes, into a staging slice on the root; ONE launch of k_aff_merge combines them entry by
 * entry (a pair lies in exactly one stretch), then the root finishes. */
int pc_multi_fill_affinity(pc_multi* m, int metric, int as_distance, const int32_t* group, int n_groups, int want_table, int64_t slab_bytes,
                           const int64_t** own_sum, const int32_t** own_lo, const int32_t** own_hi, const int32_t** near_group,
                           const int64_t** near_sum, const int32_t** near_lo, const int32_t** near_hi,
                           const int64_t** tab_sum, const int32_t** tab_lo, const int32_t** tab_hi, int32_t* n_slabs, pc_stats* stats);
/* pc_fill_hist over the devices of `m`, on the same terms and with the same deal.  Every device counts over its stretch of targets and
 * ships its raw state once, 8 (n_classes bins + 1) bytes, into a staging slice on the root; ONE launch of k_hist_merge adds them word by
 * word (a pair lies in exactly one stretch), then the root finishes.  The result is the same for any number of devices. */
int pc_multi_fill_hist(pc_multi* m, int metric, int as_distance, const int32_t* group, int n_groups, int64_t slab_bytes,
                       const int64_t** hist, int32_t* n_classes, int64_t* n_pairs, int32_t* n_slabs, pc_stats* stats);
int pc_multi_last_stretches(const pc_multi* m, int32_t* bounds /* pc_multi_devices(m) + 1 entries */);
int pc_multi_last_slab_times(const pc_multi* m, float* ms_exchange, float* ms_merge);
/* The stretch deal itself, host arithmetic only (no GPU, no context; exported for tests as pc_chunk_plan is): bounds[world + 1] with
 * bounds[0] = 0, bounds[world] = n, and for 0 < r < world bounds[r] the smallest t in [0, n] with P(t) * world >= r * P(n),
 * P(t) = cost[0] + ... + cost[t-1] (sums below 2^63; the products are 128-bit).  Non-decreasing; a stretch may be empty (world > n,
 * or zero costs).  PC_ERR_ARG: n < 0, world < 1, a NULL pointer. */
int pc_stretch_plan(const uint64_t* cost, int n, int world, int32_t* bounds);

/*
 * Test hook for the alignment kernels (replaces parasail.nw_trace_diag_16 +
 * get_traceback + the two counts read at metrics.py:216-217): aligns gene a_gene[k]
 * (rows, the reference's seq_a) against gene b_gene[k] (columns, seq_b) of the uploaded
 * genomes.  n_ident = comp.count("|"), n_diag = aligned (non-gap) columns, so
 * len(traceback.query) = la + lb - n_diag.  variant: 0 = as pc_fill would choose,
 * -1 = general fallback kernel, w > 0 = force the systolic kernel with w columns per lane
 * (every task in its class's own workgroup shape; 1000 + w: that variant with the buckets cut as pc_fill cuts
 * them -- left-over rows to the remainder chooser's variant, small tasks in one- / two-wave workgroups)
 * (a pair whose COLUMN gene holds a byte outside the 24-letter alphabet runs that variant's
 * residue-compare cell, as in pc_fill: the profile cell keeps one row for all such bytes).
 */
int pc_align_pairs(pc_ctx* ctx, const int32_t* a_gene, const int32_t* b_gene, int64_t n, int variant,
                   int32_t* n_ident, int32_t* n_diag);

/*
 * Tie-rule table of the aligner.  parasail resolves co-optimal alignments by three local rules (SURVEY.md 8c
 * item 4) that are recalled, not pinned (its source is absent); every alignment kernel exists for all 8
 * combinations, selected per context.  Bits: 1 = H prefers INS (E) over DEL (F) when both tie (default DEL first);
 * 2 = E opens when open == extend (default extends); 4 = F opens when open == extend (default extends).
 * Rule 0 is the default (build-time PC_TIE_RULE_DEFAULT, or environment PC_TIE_RULE at context creation).
 * Affects aai / peq only.  Replaces nothing in the reference: it is the handle by which a maintainer holding real
 * parasail vectors re-pins metrics.py:174-175.
 */
#define PC_NUM_TIE_RULES 8
int pc_set_tie_rule(pc_ctx* ctx, int rule);
int pc_get_tie_rule(const pc_ctx* ctx);

/* Test hook: columns per lane of the systolic variant the chooser picks for a column gene of lb residues; 0 = general kernel. */
int pc_variant_width(int lb);

/* Test hook: how the systolic kernel runs a column gene of lb residues (no byte outside the alphabet) on the variant of
 * `width` columns per lane (0: the chooser's): out[0] rows per workgroup task, out[1] waves per workgroup, out[2] row
 * streams per wave (segments; 1 when strip-mined), out[3] strip-mined passes of 64 x width columns (0: in registers).
 * An alignment stream of a full task carries out[0] / (out[1] * out[2]) alignments back to back. */
int pc_task_shape(int lb, int width, int32_t* out);

/* Test hook: how the HOST functions (variant chooser, task size, remainder chooser, task mode -- what the upload's planner
 * tables and pc_align_pairs are made from) cut a bucket of `rows` distinct row sequences against a column gene of lb residues
 * (any_byte != 0: it holds a byte outside the 24-letter alphabet): out[0] rows per task, out[1] rows that stay with the main
 * variant (they form out[1] / out[0] full tasks), out[2] launch class of a full main task (stated also when there is none),
 * out[3] launch class of the last, short main task of out[1] % out[0] rows or -1, out[4] launch class of the remainder task
 * of rows - out[1] rows or -1.  A launch class is base class * 3 + mode (0 the class's own workgroup, 1 two waves, 2 one
 * wave); base class = variant index * 4 + lanes-per-segment bucket, the same again 4 * variants higher for "any byte"
 * columns, then one per strip-mined variant (W = 32, 48, 64), then the general kernel.  Reads no device table, launches nothing. */
int pc_bucket_launch_classes(int lb, int rows, int any_byte, int32_t* out);

/* Test hook: tasks per launch class of the context's last aai / peq / aai_ppos fill (any pc_fill* route), summed over its
 * chunks, as the DEVICE planner cut them; after pc_plan_dev the whole plan's counts, after pc_align_slice_dev that slice's.
 * Writes min(cap, n) entries and returns n, the number of launch classes; PC_ERR_STATE before the first such fill. */
int pc_last_plan_tasks(const pc_ctx* ctx, int32_t* per_launch_class, int cap);

/* Test hook: columns per lane of the systolic variant a percent-positives (aai_ppos) launch runs on when the longest
 * column gene of its class has max_lb residues; 0 = the general kernel. */
int pc_ppos_width(int max_lb);

/* Test / tuning hook: HIP-event milliseconds of the alignment kernels of the last pc_align_pairs call. */
float pc_last_align_ms(const pc_ctx* ctx);

/* Which kernel family the selector gave the last gcs / jc / pocp / af fill of this context: 0 popcount tiles, 1 sparse tiles
 * 32 x 32, 2 sparse tiles 64 x 64, 3 shared-pham walker, 4 the column kernel (gcs / jc / pocp / af: target-block masks kept in LDS over a run
 * of source tiles); -1 before the first such fill.  (The selector reads the collection:
 * genomes, bitmap words, phams an average pair shares -- metrics.py:26-157 have one code path, this has four.) */
int pc_last_set_kernel(const pc_ctx* ctx);

/*
 * Test hooks: the set-metric selector and the launch shapes as host arithmetic (no GPU call, no context, no environment read).
 * The fills call the same two functions: pick the family from pc_set_inputs, then size the launch with pc_set_launch_shape.
 */
typedef enum { PC_SET_POPC = 0, PC_SET_SPARSE32 = 1, PC_SET_SPARSE64 = 2, PC_SET_WALKER = 3, PC_SET_SPARSE_COL = 4 } pc_set_family;
typedef struct pc_set_inputs {      /* what the selector reads; counted at upload, nown / max_block_entries per shard */
    int64_t n, nown;                /* genomes; target genomes this rank owns (n when unsharded)                          */
    int32_t words;                  /* bitmap words per row                                                                 */
    int32_t two_holder;             /* phams at least two genomes hold (the mask entries of the sparse kernels)            */
    double avg_shared;              /* phams an average pair shares: sum over phams of holders (holders - 1) / (n (n - 1)) */
    int32_t max_nph, max_ngen;      /* most phams, most genes of a genome                                                   */
    int32_t min_gene_len;           /* shortest translation (0: an empty one)                                               */
    int32_t max_ent_len;            /* largest summed translation length of one (genome, pham) entry                      */
    int64_t max_tlen;               /* largest summed translation length of a genome                                        */
    int64_t max_block_entries;      /* most entries of two-holder phams in one block of 64 consecutive owned targets         */
    int32_t metric;                 /* PC_GCS ... PC_AF                                                                      */
    int32_t forced;                 /* -1, or the pc_set_family that PC_SET_KERNEL names                                    */
} pc_set_inputs;
typedef struct pc_set_shape {
    int32_t family;                 /* pc_set_family                                                                        */
    int32_t tile;                   /* tile edge in genomes: 32 or 64                                                       */
    int32_t super_edge;             /* super-tile edge of the XCD-aware deal in tiles (1, 2, 4, 8, 16); 0: column kernel    */
    int32_t grid;                   /* workgroups                                                                           */
    int32_t units;                  /* tile slots (column kernel: target blocks x runs) dealt to them                       */
    int32_t units_per_wg;           /* most units one workgroup takes (1, or several on the 64 x 64 sparse tiles)           */
    int32_t chunks, chunk;          /* mask chunks and mask entries per chunk (sparse families; else 0)                     */
    int32_t batches;                /* 64 x 64 sparse tiles: 2 = one chunk holds all masks, 1 = the chunked instance        */
    int32_t dense;                  /* ... and 1 when the instance stages broadcast entries through LDS (af, two-batch)     */
    int32_t seg, runs;              /* column kernel: source tiles per unit, runs of them per target block                 */
    int32_t lds;                    /* dynamic LDS bytes of the launch                                                      */
    int32_t table;                  /* popcount tiles: 1 epilogue table, 0 division in place                                */
    int32_t vals_cap;               /* column kernel, pocp / af: entries a block's LDS value table holds (0: cannot run)    */
    int32_t reserved;
} pc_set_shape;
/* pc_set_inputs.max_block_entries as the fills count it: entries_per_genome[g] = genome g's entries of two-holder phams, owned = the
 * rank's targets, ascending; blocks of 64 consecutive owned targets, the last one ragged. */
int64_t pc_set_max_block_entries(const uint32_t* entries_per_genome, const int32_t* owned, int64_t nown);
/* The selector: the family (pc_set_family) a fill with these inputs runs on; PC_ERR_ARG for a metric that is no set metric. */
int pc_set_kernel_choice(const pc_set_inputs* in);
/* The launch shape of `family` for (metric, n, nown, words, two_holder) on a device of n_cu compute units (<= 0: 256).
 * table_top: most phams (gcs / jc) or genes (pocp) of a genome, for the popcount tiles' epilogue table.  knobs: NULL or the
 * values of PC_POPC_TILE, PC_S64_CHUNKS, PC_COL_SEG (0: unset), which the launchers read from the environment. */
int pc_set_launch_shape(int family, int metric, int64_t n, int64_t nown, int words, int two_holder, int n_cu, int table_top,
                        const int32_t* knobs, pc_set_shape* out);
/* The selector inputs and the launch shape (knobs applied) of the context's last gcs / jc / pocp / af fill; either pointer may
 * be NULL.  PC_ERR_STATE before the first such fill. */
int pc_last_set_launch(const pc_ctx* ctx, pc_set_inputs* in, pc_set_shape* shape);

/* Test hook: the device implementation of Python's round(x, 6) (the rounding every metric
 * returns through, e.g. metrics.py:50-53) applied to n host doubles in [0, 2^20). */
int pc_round6_probe(pc_ctx* ctx, const double* in, double* out, int64_t n);

/*
 * Environment switches of the library, all of them (the product needs none: defaults are what profiles/ measures).
 *
 *   read at pc_ctx_create
 *     PC_TIE_RULE=0..7          row of the aligner's tie-rule table (pc_set_tie_rule overrides it per context)
 *     PC_PLAN_BYTES=n           HBM one chunk of an aai / peq fill's plan may take (pc_set_plan_budget overrides it)
 *     PC_ALIGN_STREAMS=1..16    streams the alignment launches of a fill are dealt to (8)
 *   read once per process
 *     PC_NO_ROCTX               do not look for libroctx64 (no marker ranges)
 *     PC_UPLOAD_TIMING          per-phase wall times of pc_upload on stderr
 *     PC_RAW_STAGE_MAX=n        largest residue set staged through page-locked memory (512 MB; beyond: copied from the caller's pages)
 *   tuning / A-B switches (read once per process; every setting gives the same matrix, tests/ hold them to that)
 *     PC_TASK_BUDGET=n          cell slots per row stream of an alignment task (49,152)
 *     PC_REMAINDER=0            no narrower variant for a bucket's left-over rows
 *     PC_INC16=0|1|2            the 11- / 10-instruction DP cell wherever both are compiled (2: the 10-instruction cell also on segments of up to 64 lanes, where a workgroup shape holds its profile)
 *     PC_RATE_TABLE=0..3        which choosers read the measured rate table (pc_nw_rates.h): bit 0 variant and remainder, bit 1 the cell of a launch class (3)
 *     PC_CHOOSE_MAX_W=w         no variant wider than w columns per lane for a column gene that a narrower one holds
 *     PC_SMALL_MODES=0          no one- / two-wave workgroups for tasks of few rows;  PC_SMALL_LAUNCH_MIN=n  fewest such tasks that get a launch of their own (192)
 *     PC_FUSE=0                 one launch per launch class instead of one per register tier
 *     PC_STRIP=0                column genes beyond 4,096 residues on the one-lane-per-alignment kernel instead of strip-mined passes
 *     PC_STRIP_STREAMS=0        strip-mined launches one after the other on the caller's stream, sharing one scratch region (default: a region and a stream each)
 *     PC_SLAB_BUDGET=n          bytes the strip-mined launches' own scratch regions may take together (3 GB); what does not fit shares the first region, in line
 *     PC_LONG_PRIORITY=0        the strip-mined launches' streams at ordinary priority (default: the highest the device offers)
 *   read per fill / per launch (the tests switch them between calls)
 *     PC_POPC_TILE=32|64        force the word-split 32 x 32 / the 64 x 64 popcount tile kernel
 *     PC_SET_KERNEL=popc|sparse|sparse64|sparsecol|walker    force a kernel family for gcs / jc / pocp / af where it exists for the metric
 *     PC_S64_CHUNKS=n           at least n mask chunks in the 64 x 64 sparse tile kernel
 *     PC_COL_SEG=1..64          source tiles per unit of the column kernel (gcs / jc / pocp / af; default: by the matrix, at most 8)
 *     PC_PIPE=0|n               strip-mined launches: never pipelined (one row per wave) / always, the passes of a row over n <= 8 waves (default: by the launch's size)
 *   only in libphamclust_hip_hooks.so (compiled with -DPC_TEST_HOOKS; pc_test_hooks() == 1)
 *     PC_FAKE_OOM_ABOVE=n       device allocations above n bytes made while a fill is planning fail (fault injection)
 *     pc_hook_slab_values()     (a call, not a variable) the value triangle that stands for every filled slab of the triangular slab walks
 *     pc_hook_rows_values()     (a call, not a variable) the rows that stand for every filled slab of the rows walk (the four rows forms)
 * The Python package adds PHAMCLUST_DEVICE, PHAMCLUST_DIST_BACKEND, PHAMCLUST_DIST_MODE, PHAMCLUST_DIST_TIMEOUT_S, PHAMCLUST_LAUNCH_COST_S,
 * PHAMCLUST_FORCE_GPUS, PHAMCLUST_NO_TORCH and PHAMCLUST_NATIVE_VARIANT.
 */

#ifdef __cplusplus
}
#endif
#endif /* PHAMCLUST_HIP_H */
