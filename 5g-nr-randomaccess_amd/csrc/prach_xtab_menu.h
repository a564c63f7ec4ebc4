// prach_xtab_menu.h — the fixed menu of per-UE quantities of include/prach.h (PRACH_XTAB_ONE ... PRACH_XTAB_STATE), device side, ONE copy: what
// prach::xtab_kernel (prach_xtab.hip) bins, prach::columns_kernel (prach_columns.hip) stores and prach::pick_kernel (prach_pick.hip) filters and ranks.  xtab_value of prach_host.c is the host's statement.
#pragma once
#include "prach_device.h"

namespace prach {

// the value of a field (include/prach.h); negative: UNDEFINED.  cls: 0 idle, 1 served, 2 unserved
__device__ __forceinline__ long long xt_value(int field, const int4 &head, const int4 &tail, int nowBackoff, int ptc, int cls, int a, int E) {
    long long v = -1;
    switch (field) {
    case PRACH_XTAB_ONE: v = 0; break;
    case PRACH_XTAB_ARRIVAL: if (cls != 0) v = a; break;
    case PRACH_XTAB_SOJOURN: if (cls == 1) v = (long long)head.w + 6 - a; break;
    case PRACH_XTAB_COMPLETION: if (cls == 1) v = (long long)head.w + 6; break;
    case PRACH_XTAB_TIMER: if (cls != 0) v = head.y; break;
    case PRACH_XTAB_PTC: if (cls != 0) v = ptc; break;
    case PRACH_XTAB_FAILCOUNT: if (cls != 0) v = tail.w; break;
    case PRACH_XTAB_AGE: if (cls != 0) v = (long long)E - a; break;
    default: // STATE
        if (cls != 2) v = cls;
        else if (head.z == 1) v = nowBackoff > 0 ? 2 : 3;
        else if (head.z == 2) v = tail.y < 48 ? 4 : 5;
        else v = 6;
        break;
    }
    return v;
}
__host__ __device__ constexpr bool needs_arrival(int f) { return f == PRACH_XTAB_ARRIVAL || f == PRACH_XTAB_SOJOURN || f == PRACH_XTAB_AGE; }

// THE POLICY of this menu for the shared bodies of prach_menu_body.h: what a launch needs, the loads, the class, the value
struct XtabMenu {
    static constexpr int NCLASSES = 3; // cls is the index of the class's counter: 0 idle, 1 served, 2 unserved
    struct Needs { bool a, x, y; };    // uniform for the launch: a(i), x: nowBackoff (quarter 1), y: preambleTxCounter (quarter 2)
    static __device__ __forceinline__ Needs needs(int f) { return Needs{needs_arrival(f), f == PRACH_XTAB_STATE, f == PRACH_XTAB_PTC}; }
    static __device__ __forceinline__ Needs needs(int f, int g) { // either of two fields (the axes of a census)
        return Needs{needs_arrival(f) || needs_arrival(g), f == PRACH_XTAB_STATE || g == PRACH_XTAB_STATE, f == PRACH_XTAB_PTC || g == PRACH_XTAB_PTC};
    }
    static __device__ __forceinline__ Needs needs_raw(int w) { return Needs{false, (w >> 2) == 1, (w >> 2) == 2}; } // record word w of the columns
    struct Rec { int4 q0, q1, q2, q3; }; // q0 idx, timer, active, txTime and q3 msg2Flag, connectionRequest, msg4Flag, failCount always
    // WHOLE (the columns, for their raw words): quarters 1 and 2 as they are; otherwise the one word of each that the menu reads
    template <bool WHOLE> static __device__ __forceinline__ Rec load(const int4 *logs, int i, const Needs &n) {
        Rec r;
        r.q0 = logs[4 * (size_t)i];
        r.q3 = logs[4 * (size_t)i + 3];
        r.q1 = r.q2 = make_int4(0, 0, 0, 0);
        if (WHOLE) {
            if (n.x) r.q1 = logs[4 * (size_t)i + 1]; // firstTxTime, secondTxTime, nowBackoff, preamble
            if (n.y) r.q2 = logs[4 * (size_t)i + 2]; // preambleChange, rarWindow, maxRarCounter, preambleTxCounter
        } else {
            r.q1.z = n.x ? logs[4 * (size_t)i + 1].z : 0;
            r.q2.w = n.y ? logs[4 * (size_t)i + 2].w : 0;
        }
        return r;
    }
    static __device__ __forceinline__ int cls(const Rec &r) { return r.q0.z == -1 ? 0 : r.q3.z == 1 ? 1 : 2; }
    static __device__ __forceinline__ int bit(int cls) { return cls == 0 ? PRACH_XTAB_IDLE : cls == 1 ? PRACH_XTAB_SERVED : PRACH_XTAB_UNSERVED; }
    static __device__ __forceinline__ bool counted(int cls, int k) { return cls == k; } // whether class counter k takes this UE
    static __device__ __forceinline__ long long value(int f, const Rec &r, int cls, int a, int E) { return xt_value(f, r.q0, r.q3, r.q1.z, r.q2.w, cls, a, E); }
};

} // namespace prach
