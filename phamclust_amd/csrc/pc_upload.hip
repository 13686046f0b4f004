// pc_upload.hip -- the two upload stages of libphamclust_hip.so (part 1: the pham sets; part 2: residues, distinct sequences
// and launch classes) and the deals (pc_set_shard*, pc_shard_table, pc_target_costs; pc_stretch_plan: the stretches of pc_multi_fill_*).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <numeric>

#include "pc_host.h"

// residue byte -> code.  Alphabet letters (either case) -> 0..23 in BLOSUM62 order; every
// other byte value keeps its own identity (codes 24..229, ASCII case folded) and scores as '*'.
static void build_code_lut(uint8_t lut[256]) {
    static const char alpha[] = "ARNDCQEGHILKMFPSTWYVBZX*";
    int assigned[256];
    for (int i = 0; i < 256; ++i) assigned[i] = -1;
    for (int k = 0; k < 24; ++k) assigned[(unsigned char)alpha[k]] = k;
    int next = 24;
    for (int v = 0; v < 256; ++v) {
        if (v >= 'a' && v <= 'z') continue;
        if (assigned[v] < 0) assigned[v] = next++;
    }
    for (int v = 'a'; v <= 'z'; ++v) assigned[v] = assigned[v - 32];
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)assigned[i];
}

static int apply_shard(pc_ctx* c, int rank, int world) {
    c->plan.valid = false;                             // a plan belongs to the shard it was made for
    const int N = c->dev.N;
    std::vector<int32_t> owned; std::vector<int64_t> lbase;
    c->h_t_rank.assign(std::max(N, 1), 0); c->h_t_lbase.assign(std::max(N, 1), 0);
    int64_t best = 0;
    for (int r = 0; r < world; ++r) {
        int64_t tot = 0;
        for (int j = 0;; ++j) {
            const int pos = (j & 1) ? world - 1 - r : r;
            const int64_t t = (int64_t)j * world + pos;
            if (t >= N) { if ((int64_t)j * world >= N) break; else continue; }
            if (r == rank) { owned.push_back((int32_t)t); lbase.push_back(tot); }
            c->h_t_rank[t] = r; c->h_t_lbase[t] = tot;
            tot += t;
        }
        if (r == rank) { lbase.push_back(tot); c->shard_pairs = tot; }
        best = std::max(best, tot);
    }
    c->shard_stride = best;
    c->rank = rank; c->world = world; c->balanced = false;
    int rc = upload_vec(c->b_owned, owned); if (rc != PC_OK) return rc;
    rc = upload_vec(c->b_lbase, lbase); if (rc != PC_OK) return rc;
    c->h_owned = owned; c->h_lbase = lbase;
    c->shard.nown = (int32_t)owned.size();
    c->shard.ident = world == 1 ? 1 : 0;
    c->shard.owned = c->b_owned.as<int32_t>();
    c->shard.lbase = c->b_lbase.as<int64_t>();
    return PC_OK;
}

// Upload, part 1: everything gcs / jc / pocp / af read -- the bitmap, the rank table, the (genome, pham) entries and the
// per-genome scalars.  The reference's set metrics never touch a translation beyond its length (metrics.py:26-157), and
// encoding, hashing and ranking 10^8 residues is 90 % of a full upload.
static int upload_sets(pc_ctx* c, const pc_packed* g) {
    PcRange range("pc:upload_sets");
    int rc = PC_OK;
    const int N = g->n_genomes, P = g->n_phams, W = g->words_per_row;
    if (N <= 0 || P < 0 || W != std::max(1, (P + 63) / 64) || g->reserved != 0 || !g->bitmap || !g->nph || !g->ngen || !g->tlen ||
        !g->gene_off || !g->seq_off) {
        pc_set_error("pc_upload: inconsistent header (N=%d P=%d W=%d)", N, P, W); return PC_ERR_ARG;
    }
    const int64_t G64 = g->gene_off[N];
    if (G64 < 0 || G64 > 0x7fffffffLL || g->gene_off[0] != 0 || (G64 > 0 && (!g->gene_pham || !g->residues))) {
        pc_set_error("pc_upload: bad gene table"); return PC_ERR_ARG;
    }
    const int G = (int)G64;
    static const bool timing = getenv("PC_UPLOAD_TIMING") != nullptr;
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "pc_upload %-22s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    };
    if ((rc = wait_last_work(c, nullptr, false))) return rc;
    c->uploaded = false; c->residues_ready = false; c->target_cost.clear(); c->plan.valid = false;
    PC_HIP(hipStreamSynchronize(c->stream));
    // a new collection: a slab of scratch the last one's long genes needed (up to 4 GB: run_align_classes) is not kept for it
    // (grow-only inside a collection; nothing of the context is in flight here)
    if (c->b_scratch.cap > ((size_t)512 << 20)) c->b_scratch.release();

    // ---- host-side indices, written straight into ONE page-locked staging buffer the context keeps (grow-only) and sent with
    // ONE copy (eleven pageable copies were 1.2 of the 1.9 ms of this stage at N = 2,000).  Several threads: genomes are
    // independent once every genome knows where its entries start.
    const int Wstride = W | 1;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; };
    const size_t o_bitmap = place((size_t)N * Wstride * 8), o_rankpre = place((size_t)N * W * 4), o_gene_len = place((size_t)std::max(G, 1) * 4),
                 o_ent_off = place(((size_t)N + 1) * 4), o_nph = place((size_t)N * 4), o_ngen = place((size_t)N * 4), o_tlen = place((size_t)N * 8);
    const size_t o_ent = off;                                           // four entry arrays of E <= G elements follow
    const size_t cap_bytes = o_ent + 6 * (((size_t)std::max(G, 1) * 4 + 255) & ~(size_t)255) + (((size_t)N + 1) * 4 + 255) + (size_t)std::max(P, 1) * 4 + 1024;   // + the paralog lists + the dense-id table
    if ((rc = c->h_stage.ensure(cap_bytes))) return rc;
    uint8_t* hs = c->h_stage.as<uint8_t>();
    uint64_t* bitmap = (uint64_t*)(hs + o_bitmap); uint32_t* rankpre = (uint32_t*)(hs + o_rankpre); int32_t* gene_len_h = (int32_t*)(hs + o_gene_len);
    uint32_t* ent_off = (uint32_t*)(hs + o_ent_off); int32_t* nph_h = (int32_t*)(hs + o_nph); int32_t* ngen_h = (int32_t*)(hs + o_ngen);
    int64_t* tlen_h = (int64_t*)(hs + o_tlen);
    memcpy(nph_h, g->nph, (size_t)N * 4); memcpy(ngen_h, g->ngen, (size_t)N * 4); memcpy(tlen_h, g->tlen, (size_t)N * 8);
    std::vector<int32_t> gene_len(G);
    std::vector<int> bad(N, 0);                          // per genome: 0 ok, else the error class found by the worker
    {   // gene lengths
        std::atomic<int> over(-1);                                   // one offender to report: any will do
        parallel_chunks(G, [&](int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; ++k) {
                const int64_t len = g->seq_off[k + 1] - g->seq_off[k];
                if (len < 0 || len > 65535) { over.store((int)k, std::memory_order_relaxed); gene_len[k] = 0; } else gene_len[k] = (int32_t)len;
                gene_len_h[k] = gene_len[k];
            }
        }, 65536);                                                   // (a thread costs ~30 us to start: few of them for small inputs)
        if (over.load() >= 0) {
            const int k = over.load();
            pc_set_error("pc_upload: gene %d has length %lld (limit 65535)", k, (long long)(g->seq_off[k + 1] - g->seq_off[k])); return PC_ERR_LIMIT;
        }
    }
    int maxlen = 0, minlen = G ? 0x7fffffff : 0;
    for (int k = 0; k < G; ++k) { maxlen = std::max(maxlen, (int)gene_len[k]); minlen = std::min(minlen, (int)gene_len[k]); }
    for (int s = 0; s < N; ++s) {
        const int64_t k0 = g->gene_off[s], k1 = g->gene_off[s + 1];
        if (k1 < k0 || k1 > G) { pc_set_error("pc_upload: gene_off not monotone at genome %d", s); return PC_ERR_ARG; }
    }
    // pass 1: entries (distinct phams) per genome = popcount of its bitmap row; the gene list is checked against it in pass 2
    ent_off[0] = 0;
    parallel_chunks(N, [&](int64_t s0, int64_t s1) {
        for (int64_t s = s0; s < s1; ++s) {
            uint64_t* row = bitmap + (size_t)s * Wstride;
            memcpy(row, g->bitmap + (size_t)s * W, sizeof(uint64_t) * W);
            for (int w = W; w < Wstride; ++w) row[w] = 0;
            size_t bits = 0;
            for (int w = 0; w < W; ++w) bits += (size_t)__builtin_popcountll(row[w]);
            ent_off[(size_t)s + 1] = (uint32_t)bits;
        }
    }, 1024);
    {   // prefix sum in 64 bits, refused as soon as it passes the gene count (a malformed bitmap must not wrap the 32-bit offsets)
        uint64_t run = 0;
        for (int s = 0; s < N; ++s) {
            run += ent_off[(size_t)s + 1];
            if (run > (uint64_t)G) { pc_set_error("pc_upload: the bitmap holds more phams than there are genes"); return PC_ERR_ARG; }
            ent_off[(size_t)s + 1] = (uint32_t)run;
        }
    }
    const size_t E = ent_off[N];
    const size_t ent_stride = ((size_t)std::max<size_t>(E, 1) * 4 + 255) & ~(size_t)255;
    int32_t* ent_cnt = (int32_t*)(hs + o_ent); int32_t* ent_len = (int32_t*)(hs + o_ent + ent_stride);
    int32_t* ent_gene = (int32_t*)(hs + o_ent + 2 * ent_stride); int32_t* ent_pham = (int32_t*)(hs + o_ent + 3 * ent_stride);
    // pass 2: a genome's entries, its rank table, and the consistency checks
    parallel_chunks(N, [&](int64_t s0, int64_t s1) {
        for (int64_t s = s0; s < s1; ++s) {
            const int64_t k0 = g->gene_off[s], k1 = g->gene_off[s + 1];
            const uint64_t* row = bitmap + (size_t)s * Wstride;
            const size_t ent0 = ent_off[s], cap = ent_off[(size_t)s + 1] - ent0;
            size_t ne = 0; int64_t tl = 0; int err = 0;
            for (int64_t k = k0; k < k1 && !err;) {
                const int32_t p = g->gene_pham[k];
                if (p < 0 || p >= P || !((row[p >> 6] >> (p & 63)) & 1ULL) || (k > k0 && g->gene_pham[k - 1] >= p && g->gene_pham[k - 1] != p)) { err = 1; break; }
                int64_t k2 = k; int64_t ln = 0;
                while (k2 < k1 && g->gene_pham[k2] == p) { ln += gene_len[k2]; ++k2; }
                if (ne >= cap) { err = 2; break; }
                ent_cnt[ent0 + ne] = (int32_t)(k2 - k); ent_len[ent0 + ne] = (int32_t)ln; ent_gene[ent0 + ne] = (int32_t)k; ent_pham[ent0 + ne] = p;
                ++ne; tl += ln; k = k2;
            }
            size_t bits = 0;
            for (int w = 0; w < W; ++w) { rankpre[(size_t)s * W + w] = (uint32_t)(ent0 + bits); bits += (size_t)__builtin_popcountll(row[w]); }
            if (!err && (ne != cap || (int)ne != g->nph[s] || (int)(k1 - k0) != g->ngen[s] || tl != g->tlen[s])) err = 2;
            bad[s] = err;
        }
    }, 512);
    for (int s = 0; s < N; ++s) {
        if (bad[s] == 1) { pc_set_error("pc_upload: genome %d: a gene's pham id is out of order or not in the bitmap", s); return PC_ERR_ARG; }
        if (bad[s] == 2) { pc_set_error("pc_upload: genome %d: bitmap/nph/ngen/tlen disagree with its gene list", s); return PC_ERR_ARG; }
    }
    // phams an average genome pair shares = sum over phams of holders (holders - 1) / (N (N - 1)): what decides between the set metrics' kernels
    std::vector<uint32_t> holders((size_t)std::max(P, 1), 0u);
    {
        std::mutex merge;
        parallel_chunks((int64_t)E, [&](int64_t e0, int64_t e1) {
            std::vector<uint32_t> mine((size_t)std::max(P, 1), 0u);
            for (int64_t e = e0; e < e1; ++e) ++mine[(size_t)ent_pham[e]];
            std::lock_guard<std::mutex> lock(merge);
            for (int p2 = 0; p2 < P; ++p2) holders[(size_t)p2] += mine[(size_t)p2];
        }, 1 << 17);
        double inc = 0.0;
        for (uint32_t n : holders) inc += (double)n * (double)(n > 0 ? n - 1 : 0);
        c->avg_shared = N > 1 ? inc / ((double)N * (double)(N - 1)) : 0.0;
    }
    // paralog lists (pocp): a genome's entries with more than one gene, as (pham, count - 1).  conserved proteins of a pair =
    // 2 x shared phams + the excess counts of the shared paralog phams, and only ~6 % of the entries are paralogs
    const size_t o_para_off = (o_ent + 4 * ent_stride + 255) & ~(size_t)255;
    uint32_t* para_off = (uint32_t*)(hs + o_para_off);
    const size_t o_para = (o_para_off + ((size_t)N + 1) * 4 + 255) & ~(size_t)255;
    size_t n_para = 0;
    for (size_t e = 0; e < E; ++e) n_para += ent_cnt[e] > 1;
    const size_t para_stride = ((size_t)std::max<size_t>(n_para, 1) * 4 + 255) & ~(size_t)255;
    int32_t* para_pham = (int32_t*)(hs + o_para); int32_t* para_ex = (int32_t*)(hs + o_para + para_stride);
    {
        size_t at = 0; int max_ngen = 0;
        for (int s2 = 0; s2 < N; ++s2) {
            para_off[s2] = (uint32_t)at;
            for (size_t e = ent_off[s2]; e < ent_off[(size_t)s2 + 1]; ++e)
                if (ent_cnt[e] > 1) { para_pham[at] = ent_pham[e]; para_ex[at] = ent_cnt[e] - 1; ++at; }
            max_ngen = std::max(max_ngen, (int)g->ngen[s2]);
        }
        para_off[N] = (uint32_t)at;
        c->max_ngen = max_ngen;
        c->h_sp_n.assign((size_t)N, 0u);
        int max_ent_len = 0;
        for (int s2 = 0; s2 < N; ++s2) {
            uint32_t n = 0;
            for (size_t e = ent_off[s2]; e < ent_off[(size_t)s2 + 1]; ++e) { n += holders[(size_t)ent_pham[e]] >= 2u; max_ent_len = std::max(max_ent_len, (int)ent_len[e]); }
            c->h_sp_n[(size_t)s2] = n;
        }
        c->max_ent_len = max_ent_len;
    }
    // The 64 x 64 sparse tile kernel's own lists: only phams that at least TWO genomes hold (nothing else can be shared; in real
    // collections about half of all phams have one holder), renumbered densely in pham order, each entry as (dense id, value) pairs
    // for one 8-byte load, plus the dense ids alone (gcs / jc) and a rank table over 64-id words of the dense space -- its mask
    // chunks then cover the phams that matter, not the vocabulary.  Only the renumbering table is staged; the lists are made on the
    // device (k_sp_build, one thread per genome, each genome's kept entries at the start of its own slot of the entry arrays), as
    // are (pham, summed length) and (pham, gene count) over ALL entries in original ids for the 32 x 32 kernel (k_pair_entries).
    int P2 = 0;
    const size_t o_dense = (o_para + 2 * para_stride + 255) & ~(size_t)255;
    {
        int32_t* dense = (int32_t*)(hs + o_dense);
        for (int p2 = 0; p2 < P; ++p2) dense[p2] = holders[(size_t)p2] >= 2u ? P2++ : -1;
    }
    const int W2 = std::max(1, (P2 + 63) / 64);
    const size_t total_staged = o_dense + (((size_t)std::max(P, 1) * 4 + 255) & ~(size_t)255);
    const size_t o_pair_len = (total_staged + 255) & ~(size_t)255, o_pair_cnt = o_pair_len + 2 * ent_stride;
    const size_t o_sp_end = o_pair_cnt + 2 * ent_stride, o_sp_pham = (o_sp_end + (size_t)N * 4 + 255) & ~(size_t)255, o_sp_len = o_sp_pham + ent_stride,
                 o_sp_cnt = o_sp_len + 2 * ent_stride, o_sp_rank = o_sp_cnt + 2 * ent_stride;
    const size_t total_bytes2 = o_sp_rank + (((size_t)N * W2 * 4 + 255) & ~(size_t)255);
    lap("entries, rank table");
    if ((rc = abi_rc(c->b_sets.ensure(total_bytes2)))) return rc;
    // (an idle GPU answers its first command after 10-25 ms, whatever the command -- DMA copy, blocking copy or a copy
    // kernel all showed it when uploads followed each other with nothing in between, `tools/upload_timing.py`; that is the
    // device waking up, not this copy: behind a fill the same copy takes 0.3 ms)
    PC_HIP(hipMemcpyAsync(c->b_sets.p, hs, total_staged, hipMemcpyHostToDevice, c->stream));
    {
        uint8_t* dsb = (uint8_t*)c->b_sets.p;
        if ((rc = pc_launch_pair_entries((const int32_t*)(dsb + o_ent + 3 * ent_stride), (const int32_t*)(dsb + o_ent + ent_stride), (const int32_t*)(dsb + o_ent),
                                         (uint2*)(dsb + o_pair_len), (uint2*)(dsb + o_pair_cnt), (int64_t)E, c->stream))) return rc;
        if ((rc = pc_launch_sp_build(N, (const uint32_t*)(dsb + o_ent_off), (const int32_t*)(dsb + o_ent + 3 * ent_stride), (const int32_t*)(dsb + o_ent + ent_stride),
                                     (const int32_t*)(dsb + o_ent), (const int32_t*)(dsb + o_dense), W2, (int32_t*)(dsb + o_sp_pham), (uint2*)(dsb + o_sp_len),
                                     (uint2*)(dsb + o_sp_cnt), (uint32_t*)(dsb + o_sp_rank), (uint32_t*)(dsb + o_sp_end), c->stream))) return rc;
    }
    PC_HIP(hipStreamSynchronize(c->stream));
    lap("h2d sets");
    uint8_t* ds = (uint8_t*)c->b_sets.p;
    PcDev& d = c->dev;
    memset(&d, 0, sizeof(d));
    d.N = N; d.Wb = W; d.Wstride = Wstride; d.G = G; d.E = (int64_t)E; d.n_cu = c->n_cu;
    d.bitmap = (const uint64_t*)(ds + o_bitmap); d.rankpre = (const uint32_t*)(ds + o_rankpre);
    d.ent_cnt = (const int32_t*)(ds + o_ent); d.ent_len = (const int32_t*)(ds + o_ent + ent_stride);
    d.ent_gene = (const int32_t*)(ds + o_ent + 2 * ent_stride); d.ent_pham = (const int32_t*)(ds + o_ent + 3 * ent_stride);
    d.gene_len = (const int32_t*)(ds + o_gene_len); d.ent_off = (const uint32_t*)(ds + o_ent_off);
    d.nph = (const int32_t*)(ds + o_nph); d.ngen = (const int32_t*)(ds + o_ngen); d.tlen = (const int64_t*)(ds + o_tlen);
    d.para_off = (const uint32_t*)(ds + o_para_off); d.para_pham = (const int32_t*)(ds + o_para); d.para_ex = (const int32_t*)(ds + o_para + para_stride);
    d.ent_pair_len = (const uint2*)(ds + o_pair_len); d.ent_pair_cnt = (const uint2*)(ds + o_pair_cnt);
    d.sp_end = (const uint32_t*)(ds + o_sp_end); d.sp_pham = (const int32_t*)(ds + o_sp_pham); d.sp_len = (const uint2*)(ds + o_sp_len);
    d.sp_cnt = (const uint2*)(ds + o_sp_cnt); d.sp_rank = (const uint32_t*)(ds + o_sp_rank); d.sp_W = W2;
    c->two_holder = P2;
    c->h_gene_len.swap(gene_len);
    c->max_gene_len = maxlen; c->min_gene_len = minlen;
    c->max_nph = 0;
    c->max_tlen = 0;
    for (int s2 = 0; s2 < N; ++s2) { c->max_nph = std::max(c->max_nph, (int)g->nph[s2]); c->max_tlen = std::max(c->max_tlen, (int64_t)g->tlen[s2]); }
    c->n_residue_bytes_in = g->seq_off[G] - g->seq_off[0];
    rc = apply_shard(c, 0, 1);
    if (rc != PC_OK) return rc;
    lap("device copies (sets)");
    c->uploaded = true;
    return PC_OK;
}

// Upload, part 2: what the aligner needs -- residue codes, the distinct sequences and their ranks, the launch classes.
// g must be the packed genomes part 1 was given.
static int upload_residues(pc_ctx* c, const pc_packed* g) {
    PcRange range("pc:upload_residues");
    int rc = PC_OK;
    const int N = g->n_genomes;
    const int G = c->dev.G;
    if (N != c->dev.N || g->gene_off[N] != (int64_t)G || g->seq_off[G] - g->seq_off[0] != c->n_residue_bytes_in) {
        pc_set_error("pc_upload_residues: not the genomes pc_upload_sets was given (N %d/%d, genes %lld/%d)", N, c->dev.N, (long long)g->gene_off[N], G);
        return PC_ERR_ARG;
    }
    static const bool timing = getenv("PC_UPLOAD_TIMING") != nullptr;
    auto tick = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timing) return;
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "pc_upload %-22s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
    };
    if ((rc = wait_last_work(c, nullptr, false))) return rc;
    c->residues_ready = false; c->plan.valid = false;
    PC_HIP(hipStreamSynchronize(c->stream));
    const std::vector<int32_t>& gene_len = c->h_gene_len;
    const int maxlen = c->max_gene_len;
    std::vector<int64_t> gene_off(G);
    int64_t code_bytes = 0;
    for (int k = 0; k < G; ++k) { gene_off[k] = code_bytes; code_bytes += ((int64_t)gene_len[k] + 15) & ~15LL; }
    // The residues go to the device RAW and are encoded there (k_encode: code LUT, 16-byte padding per gene): the host only
    // hashes them -- 8 raw bytes per multiply -- and notes which genes hold a byte outside the alphabet.  (r02 encoded on the
    // host: a 10^8-byte buffer to fault in, fill through the LUT byte by byte, copy and unmap per upload.)  Hashing the raw
    // bytes means two translations that differ only in letter case count as two sequences: they are aligned twice, nothing else.
    std::vector<uint64_t> ghash(std::max(G, 1));
    std::vector<uint8_t> godd(std::max(G, 1), 0);      // gene holds a byte outside the 24-letter alphabet (code >= 24)
    uint8_t lut[256]; build_code_lut(lut);
    uint8_t is_odd[256];
    for (int v = 0; v < 256; ++v) is_odd[v] = (uint8_t)(lut[v] >= 24);
    const uint8_t* raw = g->residues;
    // The hashing threads also copy their genes' bytes into a page-locked staging buffer the context keeps (up to 512 MB;
    // beyond that the residues go over from the caller's pageable memory at the end), and the DMA to HBM is started as soon as
    // they are done: it runs behind the de-duplication and the launch-class tables below.
    const int64_t raw_bytes = g->seq_off[G] - g->seq_off[0];
    static const int64_t stage_max = getenv("PC_RAW_STAGE_MAX") ? atoll(getenv("PC_RAW_STAGE_MAX")) : ((int64_t)512 << 20);   // (test knob)
    const bool staged = raw_bytes > 0 && raw_bytes <= stage_max;
    if (staged && (rc = c->h_raw.ensure((size_t)raw_bytes))) return rc;
    if ((rc = abi_rc(c->b_raw.ensure((size_t)std::max<int64_t>(raw_bytes, 16))))) return rc;
    uint8_t* const stage = staged ? c->h_raw.as<uint8_t>() : nullptr;
    const int64_t raw0 = g->seq_off[0];
    parallel_chunks(G, [&](int64_t k0, int64_t k1) {
        if (stage) memcpy(stage + (g->seq_off[k0] - raw0), raw + g->seq_off[k0], (size_t)(g->seq_off[k1] - g->seq_off[k0]));
        for (int64_t k = k0; k < k1; ++k) {
            const uint8_t* src = raw + g->seq_off[k];
            const int len = gene_len[k];
            uint64_t h = 0x9e3779b97f4a7c15ULL ^ (uint64_t)len;
            uint8_t odd = 0;
            int i = 0;
            for (; i + 8 <= len; i += 8) {
                uint64_t w; memcpy(&w, src + i, 8);
                h = (h ^ w) * 0x9fb21c651e98df25ULL; h ^= h >> 32;
                odd |= (uint8_t)(is_odd[src[i]] | is_odd[src[i + 1]] | is_odd[src[i + 2]] | is_odd[src[i + 3]] | is_odd[src[i + 4]] | is_odd[src[i + 5]] |
                                 is_odd[src[i + 6]] | is_odd[src[i + 7]]);
            }
            uint64_t w = 0;
            for (int j = 0; i + j < len; ++j) { w |= (uint64_t)src[i + j] << (8 * j); odd |= is_odd[src[i + j]]; }
            h = (h ^ w) * 0x9fb21c651e98df25ULL; h ^= h >> 32;
            ghash[k] = h ^ (h >> 29);
            godd[k] = odd;
        }
    });
    if (staged) PC_HIP(hipMemcpyAsync(c->b_raw.p, stage, (size_t)raw_bytes, hipMemcpyHostToDevice, c->stream));
    lap("residue hashes");
    // distinct sequences (by raw residues).  Alignments are planned per distinct
    // (row sequence, column sequence) pair, so every sequence gets a rank q; ranks follow launch-class order: column
    // sequences grouped by the kernel variant that aligns against them and by lanes-per-segment bucket (the
    // profile's LDS footprint scales with it, and LDS sets occupancy)
    std::vector<int32_t> uid(G), u_gene;
    {   // Representative of a gene = the first gene with the same residues.  Sixteen hash partitions, one thread and one
        // open-addressing table each (every thread scans all hashes and takes its own: genes arrive in index order, so the first
        // one in is the first occurrence); equal hash and length are confirmed by comparing the residues.  Sequence ids then
        // follow first-occurrence order, exactly as a single serial table would number them.
        constexpr int NPART = 16;
        std::vector<int32_t> rep(G);
        std::vector<std::thread> th;
        const int nthreads = G >= 32768 ? NPART : 1;
        auto work = [&](int part, int nparts) {
            size_t cap = 16;
            while (cap < (size_t)G * 2 / (size_t)nparts + 16) cap <<= 1;
            std::vector<int32_t> slot(cap, -1);
            for (int k = 0; k < G; ++k) {
                if (nparts > 1 && (int)((ghash[k] >> 40) & (NPART - 1)) != part) continue;
                size_t pos = (size_t)ghash[k] & (cap - 1);
                for (;; pos = (pos + 1) & (cap - 1)) {
                    const int32_t r = slot[pos];
                    if (r < 0) { slot[pos] = k; rep[k] = k; break; }
                    if (ghash[r] == ghash[k] && gene_len[r] == gene_len[k] &&
                        !memcmp(raw + g->seq_off[r], raw + g->seq_off[k], (size_t)gene_len[k])) { rep[k] = r; break; }
                }
            }
        };
        if (nthreads == 1) work(0, 1);
        else {
            for (int t = 0; t < NPART; ++t) th.emplace_back(work, t, NPART);
            for (auto& x : th) x.join();
        }
        u_gene.reserve(G);
        for (int k = 0; k < G; ++k) {
            if (rep[k] == k) { uid[k] = (int32_t)u_gene.size(); u_gene.push_back(k); }
            else uid[k] = uid[rep[k]];
        }
    }
    const int U = (int)u_gene.size();
    lap("distinct sequences");
    const int ncls_all = pc_num_classes();             // last class: general kernel
    std::vector<int> u_cls(U), len_cls(maxlen + 1, -1), len_rows(maxlen + 1, 0), len_var(maxlen + 1, -1);   // per length: class, rows per task, variant
    std::vector<int64_t> cls_count(ncls_all, 0);
    for (int u = 0; u < U; ++u) {
        const int len = gene_len[u_gene[u]];
        if (len_cls[len] < 0) {
            const int variant = pc_nw_choose_variant(len);
            len_var[len] = variant;
            len_cls[len] = pc_class_of(len, variant, false);
            len_rows[len] = pc_nw_task_rows(len, variant, 0);
        }
        // A column sequence with a byte outside the alphabet goes to its variant's "any byte" class: the profile cell
        // takes "identical residues" from a profile row per alphabet letter plus ONE row for every other byte
        // (pc_nw_geometry.h, PC_INC16_MAX_W), which is exact only while the column holds none of those (as a row, it is fine)
        u_cls[u] = godd[u_gene[u]] ? pc_class_of(len, len_var[len], true) : len_cls[len]; ++cls_count[u_cls[u]];
    }
    lap("  classes per sequence");
    if (ncls_all > 250 || ncls_all * PC_WAVE_MODES + 1 > 1000) { pc_set_error("too many kernel classes"); return PC_ERR_LIMIT; }   // base class ids travel in a byte, 255 = none; the plan read-back holds 1,000 words
    c->ncls_all = ncls_all;
    std::vector<int64_t> cls_pos(ncls_all, 0);
    { int64_t run = 0; for (int cls = 0; cls < ncls_all; ++cls) { cls_pos[cls] = run; run += cls_count[cls]; } }
    std::vector<int32_t> q_gene(std::max(U, 1), 0), task_rows(std::max(U, 1), PC_TASK_ROWS);
    std::vector<uint32_t> q_of_u(std::max(U, 1), 0), gene_q(std::max(G, 1), 0);
    std::vector<uint8_t> q_class(std::max(U, 1), 0), q_nseg(std::max(U, 1), 1), rem_class((size_t)std::max(U, 1) * 16, 255);
    // per length: segments per wave of the main variant and where a remainder of r rows goes (class id, 255 = stays)
    std::vector<uint8_t> len_nseg(maxlen + 1, 1), len_rem((size_t)(maxlen + 1) * 16, 255);
    c->cls_max_lb.assign(ncls_all, 0);
    for (int len = 0; len <= maxlen; ++len) if (len_cls[len] >= 0) c->cls_max_lb[len_cls[len]] = std::max(c->cls_max_lb[len_cls[len]], len);
    for (int u = 0; u < U; ++u) if (godd[u_gene[u]]) c->cls_max_lb[u_cls[u]] = std::max(c->cls_max_lb[u_cls[u]], (int)gene_len[u_gene[u]]);
    // (the remainder chooser is a cost model evaluated ~15 times per distinct length: several threads, then the class maxima)
    parallel_chunks(maxlen, [&](int64_t l0, int64_t l1) {
        for (int64_t len = l0 + 1; len <= l1; ++len) {
            const int v = len_var[len];
            if (len_cls[len] < 0 || v < 0) continue;
            const int nseg = pc_nw_segs((int)len, pc_nw_variant_w(v));  // (a strip-mined gene: one row per wave)
            len_nseg[len] = (uint8_t)nseg;
            for (int r = 1; r < nseg; ++r) {
                const int vr = pc_nw_choose_remainder((int)len, r, v);
                if (vr >= 0) len_rem[(size_t)len * 16 + r] = (uint8_t)pc_class_of((int)len, vr, false);
            }
        }
    }, 64);
    for (int len = 1; len <= maxlen; ++len)
        for (int r = 1; r < 16; ++r) {
            const uint8_t cr = len_rem[(size_t)len * 16 + r];
            if (cr != 255) c->cls_max_lb[cr] = std::max(c->cls_max_lb[cr], len);
        }
    lap("  remainder chooser");
    // ranks inside a class follow sequence length (then first occurrence): the plan's sort then hands every bucket its
    // rows in length order, so the row streams of a task, dealt round-robin, stay in step and start their alignments
    // in the same steps (the per-step cost of an alignment start is paid once per wave, not once per segment; measured
    // gain 0.3 %: rows of one pham are nearly equally long anyway)
    std::vector<int32_t> u_order(U);
    {   // stable counting sort by length (lengths <= 65,535): a comparison sort of ~5*10^5 sequences cost 60 ms of the upload
        std::vector<int32_t> at(maxlen + 2, 0);
        for (int u = 0; u < U; ++u) ++at[gene_len[u_gene[u]] + 1];
        for (int len = 0; len <= maxlen; ++len) at[len + 1] += at[len];
        for (int u = 0; u < U; ++u) u_order[at[gene_len[u_gene[u]]]++] = u;
    }
    for (int u : u_order) q_of_u[u] = (uint32_t)cls_pos[u_cls[u]]++;        // (serial: a rank is its predecessors' count)
    lap("  ranks");
    {   // "any byte" classes a remainder may be sent to: their longest column gene (serial, rare)
        for (int u = 0; u < U; ++u) {
            const int len = gene_len[u_gene[u]];
            if (!godd[u_gene[u]] || u_cls[u] == ncls_all - 1) continue;       // (also where the MAIN variant takes any byte: a narrower remainder variant may not)
            for (int r = 1; r < 16; ++r) {
                const uint8_t cr = len_rem[(size_t)len * 16 + r];
                if (cr == 255) continue;
                const int ca = pc_class_of(len, pc_class_variant(cr), true);
                c->cls_max_lb[ca] = std::max(c->cls_max_lb[ca], len);
            }
        }
    }
    parallel_chunks(U, [&](int64_t u0, int64_t u1) {
        for (int64_t u = u0; u < u1; ++u) {
            const int q = (int)q_of_u[u];
            const int len = gene_len[u_gene[u]];
            q_gene[q] = u_gene[u];
            q_class[q] = (uint8_t)u_cls[u];
            if (u_cls[u] == ncls_all - 1) { task_rows[q] = pc_nw_task_rows(len, -1, 0); q_nseg[q] = 1; }   // general kernel (rem_class stays 255: no remainder move)
            else if (!godd[u_gene[u]]) { task_rows[q] = len_rows[len]; q_nseg[q] = len_nseg[len]; memcpy(&rem_class[(size_t)q * 16], &len_rem[(size_t)len * 16], 16); }
            else {                                                   // "any byte" column: its class's own task size, remainders to the "any byte" class of their variant
                // (also when the main variant takes any byte itself and so keeps its class, W = 32 at 641 ... 672 residues: the remainder
                // chooser sends its left-over rows to W = 11, which does not -- as pc_bucket_cut states it for pc_align_pairs)
                task_rows[q] = u_cls[u] == len_cls[len] ? len_rows[len] : pc_nw_task_rows(len, len_var[len], 1); q_nseg[q] = len_nseg[len];
                for (int r = 1; r < 16; ++r) {
                    const uint8_t cr = len_rem[(size_t)len * 16 + r];
                    if (cr == 255) continue;
                    rem_class[(size_t)q * 16 + r] = (uint8_t)pc_class_of(len, pc_class_variant(cr), true);
                }
            }
        }
    });
    parallel_chunks(G, [&](int64_t k0, int64_t k1) { for (int64_t k = k0; k < k1; ++k) gene_q[k] = q_of_u[uid[k]]; });
    int ubits = 1;
    while ((1LL << ubits) < U) ++ubits;

    lap("launch classes");
    // ---- device copies ---------------------------------------------------------------
    // The tables go through the context's page-locked staging buffer (one memcpy each, then DMA): sent with hipMemcpy straight from
    // pageable vectors, the larger ones (rem_class 16 B and gene_off 8 B per sequence) left the driver ~20 ms of deferred work
    // that the FIRST kernel launch after the upload then waited for (tools/wake_experiment.py: fill 622 ms on the host clock
    // against 599 on the device right after an upload, 599 / 599 after 50 ms of sleep).
    std::vector<int64_t> rel(g->seq_off, g->seq_off + G + 1);
    for (auto& x : rel) x -= g->seq_off[0];
    struct Item { DevBuf* buf; const void* src; size_t bytes; };
    const Item items[] = {
        {&c->b_gene_off, gene_off.data(), gene_off.size() * 8}, {&c->b_seq_tmp, rel.data(), rel.size() * 8},
        {&c->b_gene_q, gene_q.data(), gene_q.size() * 4}, {&c->b_q_gene, q_gene.data(), q_gene.size() * 4},
        {&c->b_task_rows, task_rows.data(), task_rows.size() * 4}, {&c->b_q_class, q_class.data(), q_class.size()},
        {&c->b_q_nseg, q_nseg.data(), q_nseg.size()}, {&c->b_rem_class, rem_class.data(), rem_class.size()}};
    size_t stage_total = 0;
    for (const Item& it : items) stage_total += (it.bytes + 255) & ~(size_t)255;
    if ((rc = c->h_stage.ensure(stage_total))) return rc;     // (part 1's copy out of this buffer has completed)
    uint8_t* const hs = c->h_stage.as<uint8_t>();
    const size_t codes_size = (size_t)std::max<int64_t>(code_bytes, 16);
    {
        size_t at = 0;
        for (const Item& it : items) {
            if ((rc = abi_rc(it.buf->ensure(std::max<size_t>(it.bytes, 16))))) return rc;
            if (!it.bytes) continue;
            memcpy(hs + at, it.src, it.bytes);
            PC_HIP(hipMemcpyAsync(it.buf->p, hs + at, it.bytes, hipMemcpyHostToDevice, c->stream));
            at += (it.bytes + 255) & ~(size_t)255;
        }
        // raw residues (already on their way when staged) -> codes, on the device
        PcLut lut_arg;
        memcpy(lut_arg.v, lut, 256);
        if ((!staged && (rc = upload_raw(c->b_raw, raw + g->seq_off[0], (size_t)raw_bytes))) || (rc = abi_rc(c->b_codes.ensure(codes_size))) ||
            (rc = abi_rc(c->b_cls_begin.ensure(((size_t)ncls_all * PC_WAVE_MODES + 1) * 4)))) return rc;
        if (code_bytes < 16) PC_HIP(hipMemsetAsync(c->b_codes.p, PC_PADCODE, 16, c->stream));
        rc = pc_launch_encode(c->b_raw.as<uint8_t>(), c->b_seq_tmp.as<int64_t>(), c->b_gene_off.as<int64_t>(), c->dev.gene_len, lut_arg,
                              c->b_codes.as<uint8_t>(), G, c->stream);
        hipError_t e = hipStreamSynchronize(c->stream);
        if (rc != PC_OK) return rc;
        if (e != hipSuccess) { pc_set_error("pc_upload: residue tables / encoding: %s", hipGetErrorString(e)); return PC_ERR_HIP; }
        // The raw bytes and their offsets were staging for k_encode only.  Kept (grow-only) they would double the residue footprint
        // for the life of the context and shrink what plan_budget_bytes() sees as free -- more chunks for exactly the collections
        // that are chunked; small ones keep them, so that repeated uploads do not pay a hipMalloc each (threshold 256 MB).
        if (c->b_raw.cap + c->b_seq_tmp.cap > ((size_t)256 << 20)) { c->b_raw.release(); c->b_seq_tmp.release(); }
    }
    c->task_plan.task_rows = c->b_task_rows.as<int32_t>(); c->task_plan.q_class = c->b_q_class.as<uint8_t>();
    c->task_plan.q_nseg = c->b_q_nseg.as<uint8_t>(); c->task_plan.rem_class = c->b_rem_class.as<uint8_t>();
    c->task_plan.nvar = pc_nw_num_variants(); c->task_plan.small_modes = pc_nw_small_modes_enabled(); c->task_plan.n_strip = PC_STRIP_CLASSES; c->task_plan.pad_ = 0;
    for (int v = 0; v < 32; ++v) c->task_plan.variant_w[v] = v < pc_nw_num_variants() ? pc_nw_variant_w(v) : 0;
    {   // launch classes: every base class in its three workgroup shapes, each with the base class's longest column gene
        std::vector<int32_t> per_base; per_base.swap(c->cls_max_lb);
        c->nlc = ncls_all * PC_WAVE_MODES;
        c->cls_max_lb.resize((size_t)c->nlc);
        for (int lc = 0; lc < c->nlc; ++lc) c->cls_max_lb[(size_t)lc] = per_base[(size_t)(lc / PC_WAVE_MODES)];
    }
    PcDev& d = c->dev;
    d.U = U; d.ubits = ubits; d.gene_q = c->b_gene_q.as<uint32_t>(); d.q_gene = c->b_q_gene.as<int32_t>();
    d.gene_off = c->b_gene_off.as<int64_t>(); d.codes = c->b_codes.as<uint8_t>();
    c->h_gene_odd.swap(godd);
    lap("device copies (residues)");
    c->residues_ready = true;
    return PC_OK;
}

extern "C" int pc_upload_sets(pc_ctx* c, const pc_packed* g) {
    if (!c || !g) { pc_set_error("pc_upload_sets: NULL argument"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    return upload_sets(c, g);
}
extern "C" int pc_upload_residues(pc_ctx* c, const pc_packed* g) {
    if (!c || !g) { pc_set_error("pc_upload_residues: NULL argument"); return PC_ERR_ARG; }
    if (!c->uploaded) { pc_set_error("pc_upload_residues: pc_upload_sets first"); return PC_ERR_STATE; }
    PC_ON_DEVICE(c);
    if (c->residues_ready) return PC_OK;
    return upload_residues(c, g);
}
extern "C" int pc_upload(pc_ctx* c, const pc_packed* g) {
    if (!c || !g) { pc_set_error("pc_upload: NULL argument"); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    int rc = upload_sets(c, g);
    if (rc == PC_OK) rc = upload_residues(c, g);
    if (rc != PC_OK) c->uploaded = false;
    return rc;
}

extern "C" int pc_set_shard(pc_ctx* c, int rank, int world) {
    if (!c || !c->uploaded) { pc_set_error("pc_set_shard: upload first"); return PC_ERR_STATE; }
    if (world < 1 || rank < 0 || rank >= world) { pc_set_error("pc_set_shard: rank %d of %d", rank, world); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    int rc = wait_last_work(c, nullptr, false); if (rc != PC_OK) return rc;
    PC_HIP(hipStreamSynchronize(c->stream));
    return apply_shard(c, rank, world);
}
// The COUNT walk behind the cost-balanced deals (pc_set_shard_balanced here, the stretch deal of pc_multi_fill_*): DP cells per
// target genome over all pairs, integer sums (identical on every device), kept in c->target_cost until the next upload.  The
// unsharded shard must be in force; nothing but the count buffers is written.
int pc_count_target_costs(pc_ctx* c) {
    if (!c->target_cost.empty()) return PC_OK;
    if (c->world != 1) { pc_set_error("pc_count_target_costs: context is sharded (%d/%d)", c->rank, c->world); return PC_ERR_STATE; }
    int rc = PC_OK;
    const int N = c->dev.N;
    if ((rc = c->b_cost.ensure((size_t)N * 8)) || (rc = c->b_totals.ensure(64))) return abi_rc(rc);
    PC_HIP(hipMemsetAsync(c->b_cost.p, 0, (size_t)N * 8, c->stream));
    PC_HIP(hipMemsetAsync(c->b_totals.p, 0, 64, c->stream));
    PcWalkArgs a; memset(&a, 0, sizeof(a));
    a.totals = c->b_totals.as<unsigned long long>(); a.cost_t = c->b_cost.as<unsigned long long>(); a.condensed = 1;
    if (c->dev.G > 0 && (rc = pc_launch_walk(PCW_COUNT, c->dev, c->shard, a, c->stream))) return rc;
    c->target_cost.resize(N);
    PC_HIP(hipMemcpyAsync(c->target_cost.data(), c->b_cost.p, (size_t)N * 8, hipMemcpyDeviceToHost, c->stream));
    PC_HIP(hipStreamSynchronize(c->stream));
    return PC_OK;
}

// The stretch deal of pc_multi_fill_edges / _components / _nearest as host arithmetic: contiguous stretches of targets of about
// equal summed cost (see the header).  P(t) * world >= r * P(n) in 128-bit products; P ascends, so one forward walk serves every r.
extern "C" int pc_stretch_plan(const uint64_t* cost, int n, int world, int32_t* bounds) {
    if (!cost || !bounds || n < 0 || world < 1) { pc_set_error("pc_stretch_plan: bad argument"); return PC_ERR_ARG; }
    unsigned __int128 total = 0;
    for (int t = 0; t < n; ++t) total += cost[t];
    bounds[0] = 0;
    unsigned __int128 below = 0;                       // P(t)
    int t = 0;
    for (int r = 1; r < world; ++r) {
        while (t < n && below * (unsigned)world < total * (unsigned)r) below += cost[t++];
        bounds[r] = t;
    }
    bounds[world] = n;
    return PC_OK;
}

// Cost-balanced deal.  The boustrophedon deal balances pair counts; alignment work per target genome also follows its
// gene count and how much it shares with the genomes before it.  One COUNT walk over all pairs gives the DP cells per
// target (integer sums: identical on every rank), then targets go, heaviest first, to the rank with the least work
// so far (ties: lowest rank) -- the same static, host-decided partition on every rank, no communication.
extern "C" int pc_set_shard_balanced(pc_ctx* c, int rank, int world) {
    if (!c || !c->uploaded) { pc_set_error("pc_set_shard_balanced: upload first"); return PC_ERR_STATE; }
    if (world < 1 || rank < 0 || rank >= world) { pc_set_error("pc_set_shard_balanced: rank %d of %d", rank, world); return PC_ERR_ARG; }
    PC_ON_DEVICE(c);
    int rc = wait_last_work(c, nullptr, false); if (rc != PC_OK) return rc;
    PC_HIP(hipStreamSynchronize(c->stream));
    const int N = c->dev.N;
    if (c->target_cost.empty()) {
        if ((rc = apply_shard(c, 0, 1))) return rc;                       // walk every pair
        if ((rc = pc_count_target_costs(c))) return rc;
    }
    // every pair also costs a walk visit and an output value: a floor of 2,000 cell-equivalents per pair keeps the
    // set metrics and sparse data balanced too
    std::vector<int> order(N);
    std::iota(order.begin(), order.end(), 0);
    auto cost = [&](int t) { return c->target_cost[t] + (uint64_t)t * 2000u; };
    std::sort(order.begin(), order.end(), [&](int x, int y) { return cost(x) != cost(y) ? cost(x) > cost(y) : x < y; });
    std::vector<uint64_t> load(world, 0);
    std::vector<int32_t> t_rank(std::max(N, 1), 0);
    for (int t : order) {
        int best = 0;
        for (int r = 1; r < world; ++r) if (load[r] < load[best]) best = r;
        t_rank[t] = best; load[best] += cost(t);
    }
    std::vector<int64_t> t_lbase(std::max(N, 1), 0), fill(world, 0);
    std::vector<int32_t> owned; std::vector<int64_t> lbase;
    for (int t = 0; t < N; ++t) {
        const int r = t_rank[t];
        t_lbase[t] = fill[r];
        if (r == rank) { owned.push_back(t); lbase.push_back(fill[r]); }
        fill[r] += t;
    }
    lbase.push_back(fill[rank]);
    c->shard_pairs = fill[rank];
    c->shard_stride = *std::max_element(fill.begin(), fill.end());
    c->rank = rank; c->world = world; c->balanced = true;
    if ((rc = upload_vec(c->b_owned, owned)) || (rc = upload_vec(c->b_lbase, lbase)) || (rc = upload_vec(c->b_t_rank, t_rank)) ||
        (rc = upload_vec(c->b_t_lbase, t_lbase))) return rc;
    c->h_t_rank = t_rank; c->h_t_lbase = t_lbase;
    c->h_owned = owned; c->h_lbase = lbase; c->plan.valid = false;
    c->shard.nown = (int32_t)owned.size();
    c->shard.ident = world == 1 ? 1 : 0;
    c->shard.owned = c->b_owned.as<int32_t>();
    c->shard.lbase = c->b_lbase.as<int64_t>();
    return PC_OK;
}
extern "C" int pc_shard_table(const pc_ctx* c, int32_t* t_rank, int64_t* t_lbase) {
    if (!c || !c->uploaded) { pc_set_error("pc_shard_table: upload first"); return PC_ERR_STATE; }
    if (!t_rank || !t_lbase) { pc_set_error("pc_shard_table: NULL argument"); return PC_ERR_ARG; }
    memcpy(t_rank, c->h_t_rank.data(), sizeof(int32_t) * (size_t)c->dev.N);
    memcpy(t_lbase, c->h_t_lbase.data(), sizeof(int64_t) * (size_t)c->dev.N);
    return PC_OK;
}
extern "C" int pc_target_costs(const pc_ctx* c, uint64_t* cost) {
    if (!c || !c->uploaded) { pc_set_error("pc_target_costs: upload first"); return PC_ERR_STATE; }
    if (!cost) { pc_set_error("pc_target_costs: NULL argument"); return PC_ERR_ARG; }
    if (c->target_cost.size() != (size_t)c->dev.N) { pc_set_error("pc_target_costs: no cost-balanced deal was computed for this upload (pc_set_shard_balanced)"); return PC_ERR_STATE; }
    memcpy(cost, c->target_cost.data(), sizeof(uint64_t) * (size_t)c->dev.N);
    return PC_OK;
}
extern "C" int64_t pc_shard_pairs(const pc_ctx* c) { return c && c->uploaded ? c->shard_pairs : -1; }
extern "C" int64_t pc_shard_stride(const pc_ctx* c) { return c && c->uploaded ? c->shard_stride : -1; }
