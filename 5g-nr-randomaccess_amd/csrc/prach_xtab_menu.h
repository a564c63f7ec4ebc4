// prach_xtab_menu.h — the fixed menu of per-UE quantities of include/prach.h (PRACH_XTAB_ONE ... PRACH_XTAB_STATE), device side, ONE copy: what
// prach::xtab_kernel (prach_xtab.hip) bins and prach::pick_kernel (prach_pick.hip) filters and ranks.  xtab_value of prach_host.c is the host's statement.
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

} // namespace prach
