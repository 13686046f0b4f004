// pc_nw_events.h -- the schedule of a systolic wave's flag events (pc_nw_body in pc_nw_systolic.h), as plain integer arithmetic:
// no HIP type, so that tests/test_nw_events_host.py compiles it with g++ and checks it against a brute-force list of events.
//
// A wave's row streams are staged PC_WIN = 32 entries at a time.  Two of a row's entries carry a flag, and only two lanes of a
// segment act on one: the head lane (k = 0) on RESET, at the step equal to the entry's stream position p, and the lane that holds
// column lb-1 (k = k_out <= 63) on LAST, at step p + k_out.  Whoever stages a window sees all its entries, so "does any segment's
// head or output lane meet a flag at step t" is known there, as one bit per step, and the step loop tests that bit with scalar
// instructions instead of comparing every lane's entry on the VALU.
//
// The window at stream position `base` is staged TWO steps before its first entry is due (the head lane reads its entries two steps
// ahead), i.e. while steps base-2 and base-1 of the window before are still to run.  So the pending bits are kept in a frame that
// starts at step base-2: bit j stands for step base - 2 + j, a step t tests bit (t + 2) & 31, and staging the next window moves the
// frame by 32.  A window's RESET bits then reach up to bit 2 + 31 (one 64-bit word), its LAST bits up to 2 + 31 + 63 = 96 (two).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PC_EV_FN __host__ __device__ __forceinline__
#else
#define PC_EV_FN inline
#endif

#define PC_EV_WIN 32                                        // = PC_WIN (static_assert in pc_nw_systolic.h)
#define PC_EV_LEAD 2                                        // steps between staging a window and its first entry's step

struct PcEvents {                                           // three scalar 64-bit words; frame start = (last staged base) - PC_EV_LEAD
    uint64_t rst;                                           // RESET events of head lanes
    uint64_t last_lo, last_hi;                              // LAST events at the output lane, 128 bits
};

PC_EV_FN void pc_ev_init(PcEvents& e) { e.rst = 0; e.last_lo = 0; e.last_hi = 0; }

// The frame moves on by one window: what was step bit j + 32 becomes bit j.  (The 32 bits that fall off belong to steps already run.)
PC_EV_FN void pc_ev_advance(PcEvents& e) {
    e.rst >>= PC_EV_WIN;
    e.last_lo = (e.last_lo >> PC_EV_WIN) | (e.last_hi << (64 - PC_EV_WIN));
    e.last_hi >>= PC_EV_WIN;
}

// Enter the window just staged (the frame already starts PC_EV_LEAD steps before its first position).  Bit i of resetw / lastw:
// some segment's entry at window position i carries RESET / LAST.  k_out in 0 ... 63.
PC_EV_FN void pc_ev_place(PcEvents& e, uint32_t resetw, uint32_t lastw, uint32_t k_out) {
    e.rst |= (uint64_t)resetw << PC_EV_LEAD;
    const uint32_t s = k_out + PC_EV_LEAD;                  // 2 ... 65
    const uint64_t x = lastw;
    if (s < 64) { e.last_lo |= x << s; e.last_hi |= x >> (64 - s); }
    else e.last_hi |= x << (s - 64);
}

// Does step t (>= the frame's start, < its start + 32) hold an event?
PC_EV_FN bool pc_ev_reset_at(const PcEvents& e, int t) { return (((uint32_t)e.rst >> ((uint32_t)(t + PC_EV_LEAD) & (PC_EV_WIN - 1))) & 1u) != 0; }
PC_EV_FN bool pc_ev_last_at(const PcEvents& e, int t) { return (((uint32_t)e.last_lo >> ((uint32_t)(t + PC_EV_LEAD) & (PC_EV_WIN - 1))) & 1u) != 0; }
