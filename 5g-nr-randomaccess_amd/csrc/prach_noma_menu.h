// prach_noma_menu.h — THE NOMA MENU of include/prach.h (PRACH_NOMA_ONE ... PRACH_NOMA_LOST and the four classes), device side, ONE copy: what
// prach::noma_census_kernel bins and prach::noma_columns_kernel stores (prach_noma_census.hip), and what prach::noma_summary_kernel ranks and
// prach::noma_pick_kernel filters and ranks (prach_noma_select.hip).  noma_value of prach_host.c is the host's statement.
//
// A record is four 16-byte quarters: q0 idx, timer, active, txTime | q1 firstTxTime, secondTxTime, nowBackoff, preamble | q2 preambleChange (NOMA.c: the
// sector), rarWindow, maxRarCounter (msg1ReTx), preambleTxCounter (nTxPreamble) | q3 msg2Flag, connectionRequest (msg3Wait), msg4Flag (RA), failCount
// (RaFailed | msg3Faile << 16).  The class of a UE needs q2 and q3, so every launch loads those; q0 and q1 only where a field needs them (nm_needs_q0,
// nm_needs_q1), uniform for the launch.
//
// THE BOUNDS: every menu value of a trial fits int32.  ARRIVAL, COMPLETION and AGE are subframe numbers of a NOMA.c trial of 10 000 subframes (+ 6), SOJOURN and
// LOST are at most 10 006, TIMER, PTC, RETX, SECTOR and PREAMBLE are logged int32 words, MSG3FAIL is the upper half of one, STATE is at most 8; nm_value
// computes in 64 bits.  A NEGATIVE value is UNDEFINED (the one rule of the menu).
//
// The channel gain is not a field here: it is the axis of a kind of its own (prach_run_trials_noma_gain, prach_noma_gain.hip).  With Philox the host has it
// per UE as well (prach_noma_activation_table), in the reference's stream it exists only inside the launch.
#pragma once
#include "prach_device.h"

namespace prach {

// the class bit of a UE (PRACH_NOMA_*), by precedence
__device__ __forceinline__ int nm_class(const int4 &q2, const int4 &q3) {
    return q2.x == -1 ? PRACH_NOMA_IDLE : q3.z == 1 ? PRACH_NOMA_SERVED : (q3.w & 0xffff) != 0 ? PRACH_NOMA_DROPPED : PRACH_NOMA_PENDING;
}

// the value of a field (include/prach.h); negative: UNDEFINED
__device__ __forceinline__ long long nm_value(int field, const int4 &q0, const int4 &q1, const int4 &q2, const int4 &q3, int cls, int a, int E) {
    const bool arrived = cls != PRACH_NOMA_IDLE, served = cls == PRACH_NOMA_SERVED;
    long long v = -1;
    switch (field) {
    case PRACH_NOMA_ONE: v = 0; break;
    case PRACH_NOMA_ARRIVAL: if (arrived) v = a; break;
    case PRACH_NOMA_SOJOURN: if (served) v = (long long)q0.w + 6 - a; break;
    case PRACH_NOMA_COMPLETION: if (served) v = (long long)q0.w + 6; break;
    case PRACH_NOMA_TIMER: if (arrived) v = q0.y; break;
    case PRACH_NOMA_PTC: if (arrived) v = q2.w; break;
    case PRACH_NOMA_RETX: if (arrived) v = q2.z; break;
    case PRACH_NOMA_MSG3FAIL: if (arrived) v = q3.w >> 16; break; // (arithmetic shift: a negative word is undefined)
    case PRACH_NOMA_AGE: if (arrived) v = (long long)E - a; break;
    case PRACH_NOMA_STATE:
        if (cls == PRACH_NOMA_IDLE) v = 0;
        else if (served) v = 1;
        else if (cls == PRACH_NOMA_DROPPED) v = 2;
        else if (q0.z == 1) v = q1.z > 0 ? 3 : q0.w >= E ? 4 : 5;
        else if (q0.z == 2) v = q3.y == 0 ? 6 : 7;
        else v = 8;
        break;
    case PRACH_NOMA_SECTOR: if (arrived) v = q2.x; break;
    case PRACH_NOMA_PREAMBLE: if (arrived) v = q1.w; break;
    default: // LOST: undefined where SOJOURN or TIMER is
        if (served) {
            const long long sj = (long long)q0.w + 6 - a;
            if (sj >= 0 && q0.y >= 0) v = sj - q0.y;
        }
        break;
    }
    return v;
}
__host__ __device__ constexpr bool nm_needs_arrival(int f) { return f == PRACH_NOMA_ARRIVAL || f == PRACH_NOMA_SOJOURN || f == PRACH_NOMA_AGE || f == PRACH_NOMA_LOST; }
__host__ __device__ constexpr bool nm_needs_q0(int f) {
    return f == PRACH_NOMA_SOJOURN || f == PRACH_NOMA_COMPLETION || f == PRACH_NOMA_TIMER || f == PRACH_NOMA_STATE || f == PRACH_NOMA_LOST;
}
__host__ __device__ constexpr bool nm_needs_q1(int f) { return f == PRACH_NOMA_STATE || f == PRACH_NOMA_PREAMBLE; }

// THE POLICY of this menu for the shared bodies of prach_menu_body.h: what a launch needs, the loads, the class, the value
struct NomaMenu {
    static constexpr int NCLASSES = 4; // cls is the class bit; the counters stand in the order idle, served, dropped, pending
    struct Needs { bool a, x, y; };    // uniform for the launch: a(i), x: quarter 0, y: quarter 1
    static __device__ __forceinline__ Needs needs(int f) { return Needs{nm_needs_arrival(f), nm_needs_q0(f), nm_needs_q1(f)}; }
    static __device__ __forceinline__ Needs needs(int f, int g) { // either of two fields (the axes of a census)
        return Needs{nm_needs_arrival(f) || nm_needs_arrival(g), nm_needs_q0(f) || nm_needs_q0(g), nm_needs_q1(f) || nm_needs_q1(g)};
    }
    static __device__ __forceinline__ Needs needs_raw(int w) { return Needs{false, (w >> 2) == 0, (w >> 2) == 1}; } // record word w of the columns
    struct Rec { int4 q0, q1, q2, q3; };
    template <bool WHOLE> static __device__ __forceinline__ Rec load(const int4 *logs, int i, const Needs &n) { // (a quarter is loaded whole or not at all)
        Rec r;
        r.q0 = r.q1 = make_int4(0, 0, 0, 0);
        if (n.x) r.q0 = logs[4 * (size_t)i];     // idx, timer, active, txTime
        if (n.y) r.q1 = logs[4 * (size_t)i + 1]; // firstTxTime, secondTxTime, nowBackoff, preamble
        r.q2 = logs[4 * (size_t)i + 2];           // preambleChange (sector), rarWindow, maxRarCounter, preambleTxCounter
        r.q3 = logs[4 * (size_t)i + 3];           // msg2Flag, connectionRequest, msg4Flag, failCount
        return r;
    }
    static __device__ __forceinline__ int cls(const Rec &r) { return nm_class(r.q2, r.q3); }
    static __device__ __forceinline__ int bit(int cls) { return cls; }
    static __device__ __forceinline__ bool counted(int cls, int k) { // whether class counter k takes this UE
        return cls == (k == 0 ? PRACH_NOMA_IDLE : k == 1 ? PRACH_NOMA_SERVED : k == 2 ? PRACH_NOMA_DROPPED : PRACH_NOMA_PENDING);
    }
    static __device__ __forceinline__ long long value(int f, const Rec &r, int cls, int a, int E) { return nm_value(f, r.q0, r.q1, r.q2, r.q3, cls, a, E); }
};

} // namespace prach
