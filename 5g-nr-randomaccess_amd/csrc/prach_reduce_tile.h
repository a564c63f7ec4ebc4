// prach_reduce_tile.h — what the reducer kernels share (prach_dist.hip, prach_timeline.hip, prach_sojourn.hip, prach_xtab.hip, prach_trace.hip,
// prach_summary.hip), ONE copy: the 64-bit agent-scope atomics of every flush, the job of a workgroup, the slot range of a tile of UEs with its staging
// rule, the wavefront fold of the running scalars and the flush of a group's scalar row.  Helpers and constants only; gfx950 only.
#pragma once
#include "prach_device.h"
#include "prach_slot_search.h"

namespace prach {

// relaxed, agent scope: trials of one group run on different XCDs
__device__ __forceinline__ void agent_add(unsigned long long *p, unsigned long long v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void agent_max(unsigned long long *p, unsigned long long v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the job of this workgroup (DistJob, TimelineJob, TraceJob: `wg0` is a job's first workgroup): the last one whose first workgroup is not behind it.
// Of a run of jobs with one wg0 only the last has workgroups (the others are empty), and that is the one found
template <class Job>
__device__ __forceinline__ Job job_of_workgroup(const Job *__restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].wg0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return jobs[lo];
}

// The slot range of a tile of consecutive UEs [first, end) of a TimelineJob.  UEs are activated in index order, so the arrival slots of a tile are one
// contiguous range [slo, shi] of the schedule: its two ends come from a search over the whole schedule, the range is staged in LDS when it has at most
// TILE_SCHED_CAP entries (a longer one is searched in global memory), and every UE's own slot comes from a search inside it.
constexpr int TILE_SCHED_CAP = 2048;
constexpr int TL_SCHED_CAP = TILE_SCHED_CAP, SJ_SCHED_CAP = TILE_SCHED_CAP, XT_SCHED_CAP = TILE_SCHED_CAP; // the names the kernels' harnesses print it under
struct TileSlots {
    int slo, shi;    // the same in every thread
    const int *sp;   // sp[0] is the entry of slot sbase: the staged range, or the job's schedule
    int sbase;
    __device__ __forceinline__ int arrival(const TimelineJob &J, int i) const { return J.aT * first_slot_above(sp, sbase, slo, shi, i); } // a(i) of include/prach.h
};
// lsched: TILE_SCHED_CAP words of LDS; every thread of the workgroup calls, and the CALLER's barrier stands between this copy and the first arrival()
template <int THREADS>
__device__ __forceinline__ TileSlots tile_slots(const TimelineJob &J, int first, int end, int *lsched, int tid) {
    const int slo = first_slot_above(J.sched, 0, 0, J.nslots, first);
    const int shi = first_slot_above(J.sched, 0, slo, J.nslots, end - 1);
    if (shi - slo > TILE_SCHED_CAP) return TileSlots{slo, shi, J.sched, 0};
    for (int s = tid; s < shi - slo; s += THREADS) lsched[s] = J.sched[slo + s];
    return TileSlots{slo, shi, lsched, slo};
}

// a wavefront's values folded into lane 0 (the other lanes hold partial results: not prach_device_fn.h's wave_sum / wave_max, whose DPP scan leaves
// a wave-uniform result and takes int only)
template <class T> __device__ __forceinline__ T fold_sum(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}
template <class T> __device__ __forceinline__ T fold_max(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (T)__shfl_down(v, d));
    return v;
}

// the scalar epilogue: a workgroup's LDS scalars into its group's row, `nsum` sums in front and `nmax` maxima behind them (the two counts stand next to
// every kernel's *_SCALARS in prach_device.h), only where non-zero
__device__ __forceinline__ void flush_scalars(const unsigned long long *lsc, unsigned long long *gsc, int nsum, int nmax, int tid) {
    if (tid >= nsum + nmax || !lsc[tid]) return;
    if (tid < nsum) agent_add(&gsc[tid], lsc[tid]); else agent_max(&gsc[tid], lsc[tid]);
}

} // namespace prach
