// Stand-alone check of phamclust_amd/csrc/pc_nw_events.h (built and run by tests/test_nw_events_host.py, under ASan + UBSan).
// A wave of the systolic kernel is replayed as far as its flag events go: the streams' entries are staged window by window at
// the steps pc_nw_body stages them, their flags go through pc_ev_advance / pc_ev_place, and at every step pc_ev_reset_at /
// pc_ev_last_at must say exactly what a brute-force list of (step, event) says -- no event missed, none reported twice or early.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pc_nw_events.h"

enum : uint32_t { F_LAST = 0x100, F_RESET = 0x200 };

struct Stream { std::vector<uint32_t> flags; };          // one entry per stream position: a virtual row -1 (RESET), then the row (LAST on its end)

static Stream make_stream(const std::vector<int>& rows) {
    Stream s;
    for (int la : rows) {
        s.flags.push_back(F_RESET);
        for (int i = 0; i < la; ++i) s.flags.push_back(i == la - 1 ? F_LAST : 0u);
    }
    return s;
}

static uint32_t g_rng = 12345u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }

static long g_cases = 0, g_bad = 0, g_events = 0;
static int g_max_windows = 0;

// k_out: the output lane; G: lanes per segment (> k_out), which only sets how many steps run
static void run_case(const std::vector<Stream>& segs, int k_out, int G) {
    int maxlen = 0;
    for (const Stream& s : segs) maxlen = (int)s.flags.size() > maxlen ? (int)s.flags.size() : maxlen;
    if (maxlen == 0) return;                               // (a wave without rows leaves the kernel before the step loop)
    int T = maxlen + G - 1;
    T += T & 1;                                            // the loop runs two steps per iteration
    std::vector<uint8_t> want_rst(T, 0), want_last(T, 0);  // brute force
    for (const Stream& s : segs)
        for (size_t p = 0; p < s.flags.size(); ++p) {
            if ((s.flags[p] & F_RESET) && (int)p < T) want_rst[p] = 1;
            if ((s.flags[p] & F_LAST) && (int)p + k_out < T) want_last[p + k_out] = 1;
        }
    PcEvents ev;
    pc_ev_init(ev);
    int windows = 0;
    auto refill = [&](int base) {
        uint32_t resetw = 0, lastw = 0;
        for (const Stream& s : segs)
            for (int i = 0; i < PC_EV_WIN; ++i) {
                const size_t p = (size_t)base + (size_t)i;
                const uint32_t f = p < s.flags.size() ? s.flags[p] : 0u;
                if (f & F_RESET) resetw |= 1u << i;
                if (f & F_LAST) lastw |= 1u << i;
            }
        if (base != 0) pc_ev_advance(ev);
        pc_ev_place(ev, resetw, lastw, (uint32_t)k_out);
        ++windows;
    };
    refill(0);
    bool bad = false;
    for (int t = 0; t < T; ++t) {
        if ((t & 1) == 0 && ((t + PC_EV_LEAD) & (PC_EV_WIN - 1)) == 0) refill(t + PC_EV_LEAD);
        const bool r = pc_ev_reset_at(ev, t), l = pc_ev_last_at(ev, t);
        g_events += r + l;
        if (r != (want_rst[t] != 0) || l != (want_last[t] != 0)) {
            if (!bad && g_bad < 10) std::printf("MISMATCH k_out %d G %d segments %zu step %d: reset %d (want %d) last %d (want %d)\n", k_out, G, segs.size(), t, (int)r, (int)want_rst[t], (int)l, (int)want_last[t]);
            bad = true;
        }
    }
    ++g_cases;
    g_bad += bad;
    if (windows > g_max_windows) g_max_windows = windows;
}

int main() {
    const int NSEG[3] = {1, 2, 16};
    const int EDGE[8] = {1, 2, 31, 32, 33, 63, 64, 65};     // row lengths around the window size and twice it
    for (int k_out = 0; k_out < 64; ++k_out) {
        // one segment, streams of 1 ... 5 rows of one length, every length 1 ... 70 (5 x 71 positions: twelve windows)
        for (int la = 1; la <= 70; ++la)
            for (int rows = 1; rows <= 5; ++rows) run_case({make_stream(std::vector<int>(rows, la))}, k_out, k_out + 1);
        // 1, 2 and 16 segments of mixed rows; some segments empty (fewer rows than segments); G from k_out + 1 up to 64
        for (int ns = 0; ns < 3; ++ns)
            for (int trial = 0; trial < 40; ++trial) {
                std::vector<Stream> segs;
                for (int s = 0; s < NSEG[ns]; ++s) {
                    std::vector<int> rows;
                    const int n = (s > 0 && rnd(4) == 0) ? 0 : 1 + (int)rnd(5);
                    for (int q = 0; q < n; ++q) rows.push_back(trial % 2 ? 1 + (int)rnd(70) : EDGE[rnd(8)]);
                    segs.push_back(make_stream(rows));
                }
                run_case(segs, k_out, k_out + 1 + (int)rnd((uint32_t)(64 - k_out)));
            }
    }
    std::printf("cases %ld events %ld max_windows %d mismatches %ld\n", g_cases, g_events, g_max_windows, g_bad);
    return g_bad ? 1 : 0;
}
