// pc_nw.hip -- K4: batched global alignment (Needleman-Wunsch, affine gaps 11/1,
// BLOSUM62) producing only what the reference reads from each alignment
// (metrics.py:216-217): n_ident = comp.count("|") and len(traceback.query).
//
// Replaces parasail.nw_trace_diag_16 + get_traceback (metrics.py:174-175).  No trace
// table is stored: the traceback's choice at every cell is a deterministic local rule
// (SURVEY.md 8c items 4-5), so (n_ident, n_diag) ride along with H, E and F in one
// forward pass and aln_len = la + lb - n_diag.
//   E(i,j) = max(H(i,j-1)-11, E(i,j-1)-1)   ties -> extend      (gap in query, "INS")
//   F(i,j) = max(H(i-1,j)-11, F(i-1,j)-1)   ties -> extend      (gap in ref,   "DEL")
//   H(i,j) = max(H(i-1,j-1)+S, E, F)        ties -> DIAG, then F, then E
// Those three tie-breaks are rule 0 of the TIE-RULE TABLE below (PcTag / pc_cell): parasail's source is not available
// (SURVEY.md 8c), so each is a switch -- every kernel exists for all 8 combinations and pc_set_tie_rule() picks
// one at run time (the CPU checker under tests/ has the same switch).  tests/golden/tie_sensitivity.json holds
// what each switch is worth.
// Scores are kept as Ho = H - 11 ("already opened"), which is what both E of the next
// column and F of the next row consume; the substitution profile is biased by +11.
// Stats are one u32: n_ident in the low half, n_diag in the high half, so the diagonal
// update is a single add-with-carry: SD = SHdiag + 0x10000 + (a == b).
// In the systolic kernel score, tie-break tag and stats travel as ONE 64-bit word and v_max_f64 is the
// lexicographic max over them (see "The DP cell as a LEXICOGRAPHIC MAX" below).
// VALU work: no MFMA (there is no dense contraction in this recurrence).
// This unit: the general kernel and the launchers.  Which variant, cell and workgroup shape a launch takes is host arithmetic of its
// own (pc_nw_shape.hip), handed over as a PcLaunchShape.
#include "pc_nw_systolic.h"     // the systolic kernel (shared with pc_nw_rules.hip), BLOSUM62
#include <algorithm>
#include <utility>

// One DP cell in the Ho convention.  In:  Hol/El/SHl/SEl from (i,j-1), Hou/Fu/SHu/SFu from
// (i-1,j), Hod/SHd from (i-1,j-1), sp = S(a_i,b_j)+11, eq = (a_i == b_j).  Out: Ho,E,F,SH,SE,SF.
struct PcCell { int Ho, E, F; uint32_t SH, SE, SF; };

// TIE-RULE TABLE (bits of `rule`; include/phamclust_hip.h documents the same numbering):
//   bit 0  H takes a gap state and E == F:   0: F (DEL) before E (INS)        1: E before F
//   bit 1  E: open == extend:                0: extend (open iff strictly >)  1: open
//   bit 2  F: open == extend:                0: extend                        1: open
// DIAG always wins a tie with a gap state.  This C++ cell (general kernel) reads the rule at run time; the
// systolic kernel spells the rule as tags of its 64-bit words (PcTag<RULE> below).
__device__ __forceinline__ PcCell pc_cell(int Hol, int El, uint32_t SHl, uint32_t SEl, int Hou, int Fu, uint32_t SHu,
                                          uint32_t SFu, int Hod, uint32_t SHd, int sp, bool eq, int rule) {
    PcCell c;
    const int Ee = El - PC_EXT, Fe = Fu - PC_EXT;
    c.E = max(Hol, Ee);
    c.SE = ((rule & 2) ? Hol >= Ee : Hol > Ee) ? SHl : SEl;
    c.F = max(Hou, Fe);
    c.SF = ((rule & 4) ? Hou >= Fe : Hou > Fe) ? SHu : SFu;
    const int D = Hod + sp;
    const int H = max(max(D, c.E), c.F);
    const uint32_t SD = SHd + 0x10000u + (eq ? 1u : 0u);
    const uint32_t ST = (rule & 1) ? ((H == c.E) ? c.SE : c.SF) : ((H == c.F) ? c.SF : c.SE);   // flat selects: nested ?: becomes control flow
    c.SH = (H == D) ? SD : ST;
    c.Ho = H - PC_OPEN;
    return c;
}

// ---------------------------------------------------------------------------------
// General kernel: any lengths.  One workgroup (one wave) per task, one lane per row
// sequence, all lanes share the task's column sequence b (so b_j is wave-uniform and
// the per-column state of 64 alignments is one coalesced 1 KiB line in HBM scratch).
// Used for column sequences longer than the systolic variants cover, and by tests.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_nw_general(PcDev d, const PcTask* __restrict__ tasks, int ntasks,
                                                   const int32_t* __restrict__ bucket_row,
                                                   const uint32_t* __restrict__ bucket_dest, uint2* __restrict__ res,
                                                   int4* __restrict__ scratch, int64_t scratch_stride, int ppos, int rule) {
    __shared__ int8_t tab[24][24];
    for (int i = threadIdx.x; i < 576; i += 64) tab[i / 24][i % 24] = (int8_t)(c_b62[i / 24][i % 24] + PC_OPEN);
    __syncthreads();
    int4* sc = scratch + (int64_t)blockIdx.x * scratch_stride;
    const int lane = threadIdx.x;
    for (int task = blockIdx.x; task < ntasks; task += gridDim.x) {
        const PcTask tk = tasks[task];
        const int lb = d.gene_len[tk.gene];
        const uint8_t* bp = d.codes + d.gene_off[tk.gene];
      for (int base = tk.begin; base < tk.end; base += 64) {       // a task may hold up to PC_TASK_ROWS rows
        const int row = base + lane;
        const bool active = row < tk.end;
        int la = 0; const uint8_t* ap = nullptr;
        if (active) { const int ga = bucket_row[row]; la = d.gene_len[ga]; ap = d.codes + d.gene_off[ga]; }
        int la_max = la;
        for (int o = 32; o > 0; o >>= 1) la_max = max(la_max, __shfl_xor(la_max, o));
        // row -1: Ho(-1,j) = -(11 + j) - 11, F = -inf, stats 0
        for (int j = 0; j < lb; ++j) sc[(int64_t)j * 64 + lane] = make_int4(-(PC_OPEN + j * PC_EXT) - PC_OPEN, PC_NEG, 0, 0);
        uint32_t final_stat = 0;
        for (int i = 0; i < la_max; ++i) {
            const bool live = i < la;
            const int ai = live ? ap[i] : 0;
            const int8_t* trow = tab[min(ai, 23)];
            int Hol = -(PC_OPEN + i * PC_EXT) - PC_OPEN, El = PC_NEG;
            uint32_t SHl = 0, SEl = 0;
            int Hod = (i == 0 ? 0 : -(PC_OPEN + (i - 1) * PC_EXT)) - PC_OPEN;
            uint32_t SHd = 0;
            for (int j = 0; j < lb; ++j) {
                const int bj = bp[j];
                const int4 up = sc[(int64_t)j * 64 + lane];
                const PcCell c = pc_cell(Hol, El, SHl, SEl, up.x, up.y, (uint32_t)up.z, (uint32_t)up.w, Hod, SHd,
                                         trow[min(bj, 23)], ai == bj || (ppos && trow[min(bj, 23)] > PC_OPEN), rule);   // ppos: '+' columns count too
                if (live) sc[(int64_t)j * 64 + lane] = make_int4(c.Ho, c.F, (int)c.SH, (int)c.SF);
                Hod = up.x; SHd = (uint32_t)up.z;
                Hol = c.Ho; El = c.E; SHl = c.SH; SEl = c.SE;
            }
            if (i == la - 1) final_stat = SHl;
        }
        if (active) {
            const uint32_t ident = final_stat & 0xffffu, ndiag = final_stat >> 16;
            res[bucket_dest ? bucket_dest[row] : (uint32_t)row] = make_uint2(ident, (uint32_t)(la + lb) - ndiag);
        }
      }
    }
}
// Tie rules 2..7 of the systolic kernel are instantiated in pc_nw_rules.hip (three objects): not here
#define PC_EXT1R(W, R) extern template int pc_systolic_launch<W, R, false> PC_SYSTOLIC_SIG;
#define PC_EXT1(W) PC_EXT1R(W, 2) PC_EXT1R(W, 3) PC_EXT1R(W, 4) PC_EXT1R(W, 5) PC_EXT1R(W, 6) PC_EXT1R(W, 7)
#define PC_EXT_TIER_R(T, R) extern template int pc_tier_launch<T, R, false> PC_TIER_SIG; extern template int pc_tier_launch<T, R, true> PC_TIER_SIG;
#define PC_EXT_TIER(T) PC_EXT_TIER_R(T, 2) PC_EXT_TIER_R(T, 3) PC_EXT_TIER_R(T, 4) PC_EXT_TIER_R(T, 5) PC_EXT_TIER_R(T, 6) PC_EXT_TIER_R(T, 7)
PC_FOR_TIER(PC_EXT_TIER)
PC_FOR_W1(PC_EXT1)
#define PC_EXT_STRIP_R(W, INC, R) extern template int pc_strip_launch<W, R, INC> PC_STRIP_SIG;
#define PC_EXT_STRIP(W, INC) PC_EXT_STRIP_R(W, INC, 2) PC_EXT_STRIP_R(W, INC, 3) PC_EXT_STRIP_R(W, INC, 4) PC_EXT_STRIP_R(W, INC, 5) PC_EXT_STRIP_R(W, INC, 6) PC_EXT_STRIP_R(W, INC, 7)
PC_EXT_STRIP(32, false) PC_EXT_STRIP(48, false) PC_EXT_STRIP(64, false) PC_EXT_STRIP(24, true) PC_EXT_STRIP(8, false) PC_EXT_STRIP(12, false)
#define PC_EXT_PIPE_R(W, R) extern template int pc_strip_launch<W, R, false, true> PC_STRIP_SIG;
#define PC_EXT_PIPE(W) PC_EXT_PIPE_R(W, 2) PC_EXT_PIPE_R(W, 3) PC_EXT_PIPE_R(W, 4) PC_EXT_PIPE_R(W, 5) PC_EXT_PIPE_R(W, 6) PC_EXT_PIPE_R(W, 7)
PC_EXT_PIPE(PC_STRIP_W_ONE_ROW)

// A wave of the systolic kernel keeps at most 64 rows (pc_nw_body: a lane-indexed row table) and takes ceil(R / (nw nseg)) nseg of a
// task's R rows: nw waves hold any task of up to nw x min over nseg of floor(64 / nseg) nseg = nw x 52 rows (nseg = 13).  The planner
// cuts tasks to the CLASS's waves per workgroup and to PC_TASK_ROWS (pc_nw_task_rows); the LAUNCH's waves are worked out on their own
// (cell, percent-positives variant swap, small-task modes).  Should the two ever drift apart, rows beyond a wave's 64 would be dropped
// without a fault -- their result slots left unwritten -- so every launch checks: tasks in their class's own shape need 52 nw >=
// PC_TASK_ROWS, i.e. four waves; the one- / two-wave modes hold tasks of at most nseg / 2 nseg rows by construction (pc_nw_task_mode).
static_assert(PC_TASK_ROWS <= 4 * 52, "four-wave workgroups must hold a full-size task");
static bool pc_launch_holds_task_rows(int nw, int wave_mode) { return wave_mode != PC_MODE_CLASS || nw * 52 >= PC_TASK_ROWS; }

// A run-time value as a compile-time constant: fn(std::integral_constant<int, I>) for the I of the list that v is.
// (A LEFT fold: it instantiates fn front to back, and the kernels lie in the code object in the order of their instantiation.)
template <class F, int... I> static void with_constant(int v, std::integer_sequence<int, I...>, F&& fn) {
    (void)(... || (v == I && (fn(std::integral_constant<int, I>{}), true)));
}
static bool tie_rule_ok(int rule) { if (rule >= 0 && rule < PC_NUM_TIE_RULES) return true; pc_set_error("tie rule %d out of range 0..7", rule); return false; }
// One launch as an instantiation: `form` (one of `forms`: the shape unit names compiled kernels only) and the tie rule as compile-time
// constants; launch(form, rule) returns the launch's hipError_t.  `kernel`, `param` name it in the message.
template <class L, class F> static int launch_as(int form, L forms, int rule, const char* kernel, int param, F&& launch) {
    if (!tie_rule_ok(rule)) return PC_ERR_ARG;
    hipError_t e = hipErrorInvalidValue;
    with_constant(form, forms, [&](auto S) { with_constant(rule, std::make_integer_sequence<int, PC_NUM_TIE_RULES>{}, [&](auto R) { e = (hipError_t)launch(S, R); }); });
    if (e != hipSuccess) { pc_set_error("%s<%d,%d> launch: %s", kernel, param, rule, hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}

// One launch over several launch classes of one fuse key (pc_nw_fuse_key): `segs` = (first task, tasks, variant, longest column
// gene, compare-only, wave mode) each, at most PC_FUSE_MAX_SEG of them, tasks taken from task_list.
int pc_launch_nw_group(const PcNwSegment* segs, int nsegs, const PcDev& d, const PcTask* task_list, const int32_t* bucket_row,
                       const uint32_t* bucket_dest, uint2* res, int ppos, int rule, hipStream_t st) {
    if (nsegs <= 0) return PC_OK;
    if (nsegs > PC_FUSE_MAX_SEG) { pc_set_error("pc_launch_nw_group: %d segments (limit %d)", nsegs, PC_FUSE_MAX_SEG); return PC_ERR_ARG; }
    PcFuseArgs f; memset(&f, 0, sizeof(f));
    int tier = -1, nw = 0; bool inc16 = false; size_t lds = 0; uint32_t blocks = 0;
    for (int i = 0; i < nsegs; ++i) {
        const PcNwSegment& sg = segs[i];
        const int W = pc_nw_variant_w(sg.variant), t = pc_tier_of(W);
        if (W == 0 || sg.max_lb > 64 * W || t < 0) {
            pc_set_error("pc_launch_nw_group: variant %d with %d columns has no tier kernel", sg.variant, sg.max_lb); return PC_ERR_ARG;
        }
        PcLaunchShape sh;
        int rc = pc_nw_launch_shape(sg.variant, sg.max_lb, ppos, sg.compare_only, sg.wave_mode, (int)sg.ntasks, d.n_cu, sh);
        if (rc != PC_OK) return rc;
        if (!pc_launch_holds_task_rows(sh.nw, sg.wave_mode)) { pc_set_error("pc_launch_nw_group: %d-wave workgroups cannot hold the rows of a full-size task (variant %d, %d columns)", sh.nw, sg.variant, sg.max_lb); return PC_ERR_STATE; }
        if (i == 0) { tier = t; nw = sh.nw; inc16 = sh.inc16; }
        else if (t != tier || sh.nw != nw || sh.inc16 != inc16) { pc_set_error("pc_launch_nw_group: segments of different tier / cell / workgroup size"); return PC_ERR_ARG; }
        lds = std::max(lds, sh.lds);
        blocks += sg.ntasks;
        f.block_end[i] = blocks; f.task_begin[i] = sg.task_begin; f.w[i] = W;
    }
    f.nseg = nsegs;
    if (blocks == 0) return PC_OK;
    // the tier's profile-cell kernel, then its compare one
    return launch_as(tier * 2 + (inc16 ? 0 : 1), std::make_integer_sequence<int, 2 * PC_NUM_TIERS>{}, rule, "k_nw_systolic_tier", tier, [&](auto F, auto R) {
        return pc_tier_launch<decltype(F)::value / 2, decltype(R)::value, decltype(F)::value % 2 == 0>(blocks, nw, lds, st, d, task_list, f, bucket_row, bucket_dest, res, ppos);
    });
}

int pc_launch_nw(int variant, const PcDev& d, const PcTask* tasks, int ntasks, const int32_t* bucket_row,
                 const uint32_t* bucket_dest, uint2* res, void* scratch, size_t scratch_bytes, int max_lb, int ppos, int rule, int compare_only, hipStream_t st,
                 int wave_mode, int max_row_len) {
    if (ntasks <= 0) return PC_OK;
    if (variant >= 0 && ppos && !pc_nw_ppos_systolic(variant, max_lb)) { pc_set_error("pc_launch_nw: percent-positives cannot run on variant %d for %d columns", variant, max_lb); return PC_ERR_ARG; }
    if (variant >= 0) {
        const int Wv = pc_nw_variant_w(variant);
        if (Wv == 0) { pc_set_error("pc_launch_nw: no variant %d", variant); return PC_ERR_ARG; }
        if (pc_tier_of(Wv) >= 0 && !pc_nw_launch_is_strip(variant, max_lb, wave_mode, ppos)) {      // a tier kernel with this one class as its only segment
            PcNwSegment sg; sg.task_begin = 0; sg.ntasks = (uint32_t)ntasks; sg.variant = variant; sg.max_lb = max_lb; sg.compare_only = compare_only; sg.wave_mode = wave_mode;
            return pc_launch_nw_group(&sg, 1, d, tasks, bucket_row, bucket_dest, res, ppos, rule, st);
        }
        PcLaunchShape sh;
        const int rc = pc_nw_launch_shape(variant, max_lb, ppos, compare_only, wave_mode, ntasks, d.n_cu, sh);
        if (rc != PC_OK) return rc;
        if (sh.strip) {      // strip-mined passes (k_nw_strip) in the form the shape says: a persistent grid of as many workgroups as the scratch holds boundary lines for
            const size_t per = pc_strip_block_bytes(max_row_len, sh.nw);
            size_t blocks = scratch ? scratch_bytes / per : 0;
            if (blocks == 0) { pc_set_error("k_nw_strip<%d>: needs %zu bytes of scratch per workgroup", sh.W, per); return PC_ERR_ARG; }
            const size_t units = (size_t)ntasks * (sh.pipe ? PC_STRIP_WAVES : 1);     // (pipelined: a workgroup per row)
            blocks = std::min(std::min(blocks, units), (size_t)4096);
            // its compiled forms: 0 = pipelined narrow passes, 1 = the profile cell's widest variant, else the compare cell at that width
            return launch_as(sh.pipe ? 0 : sh.inc16 ? 1 : sh.W, std::integer_sequence<int, 0, 1, PC_STRIP_W_ONE_ROW, PC_STRIP_W_TWO_ROWS, 32, 48, 64>{}, rule, "k_nw_strip", sh.W, [&](auto F, auto R) {
                constexpr int f = decltype(F)::value, W = f == 0 ? PC_STRIP_W_ONE_ROW : f == 1 ? PC_INC16_MAX_W : f;
                return pc_strip_launch<W, decltype(R)::value, f == 1, f == 0>((unsigned)blocks, sh.nw, sh.lds, st, d, tasks, ntasks, bucket_row, bucket_dest, res, sh.inc16 ? 1 : 0,
                                                                              (uint4*)scratch, (unsigned)(max_row_len + 2));
            });
        }
        // the wide variants (W = 32, 48, 64): a kernel each
        if (!pc_launch_holds_task_rows(sh.nw, wave_mode)) { pc_set_error("k_nw_systolic<%d>: %d-wave workgroups cannot hold the rows of a full-size task", sh.W, sh.nw); return PC_ERR_STATE; }
        return launch_as(sh.W, std::integer_sequence<int, 32, 48, 64>{}, rule, "k_nw_systolic", sh.W, [&](auto W, auto R) {
            return pc_systolic_launch<decltype(W)::value, decltype(R)::value, false>((unsigned)ntasks, sh.nw, sh.lds, st, d, tasks, bucket_row, bucket_dest, res, 0);
        });
    }
    if (!tie_rule_ok(rule)) return PC_ERR_ARG;
    // general kernel: one scratch slab of 64 * max_lb cells per resident workgroup
    const size_t per_block = (size_t)64 * (size_t)(max_lb > 0 ? max_lb : 1) * sizeof(int4);
    size_t blocks = scratch ? scratch_bytes / per_block : 0;
    if (blocks == 0) { pc_set_error("pc_launch_nw: general kernel needs %zu bytes of scratch per workgroup", per_block); return PC_ERR_ARG; }
    if (blocks > 1024) blocks = 1024;
    if (blocks > (size_t)ntasks) blocks = (size_t)ntasks;
    hipLaunchKernelGGL(k_nw_general, dim3((unsigned)blocks), dim3(64), 0, st, d, tasks, ntasks, bucket_row, bucket_dest, res,
                       (int4*)scratch, (int64_t)(per_block / sizeof(int4)), ppos, rule);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pc_set_error("k_nw_general launch: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
    return PC_OK;
}
