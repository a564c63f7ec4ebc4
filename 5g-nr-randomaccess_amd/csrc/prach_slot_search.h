// prach_slot_search.h — the search over a trial's arrival schedule that the reductions reading per-UE log records share (prach_timeline.hip,
// prach_sojourn.hip): a(i) of include/prach.h is accessTime x first_slot_above(sched, ..., i).  ONE copy.
#pragma once
#include <hip/hip_runtime.h>

namespace prach {

// the first slot in [lo, hi] whose schedule entry exceeds i; hi itself is never read (it may be the slot count: no slot activates the UE).
// sched[0] is the entry of slot `base` (a staged range starts at the tile's first slot: an LDS pointer is never moved below its array)
__device__ __forceinline__ int first_slot_above(const int *sched, int base, int lo, int hi, int i) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sched[mid - base] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

} // namespace prach
