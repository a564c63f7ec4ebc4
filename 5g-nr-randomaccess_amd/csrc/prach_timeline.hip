// prach_timeline.hip — prach::timeline_kernel: per trial group, what arrived, was served and completed in each stretch of the simulation
// (include/prach.h, prach_run_trials_timeline), reduced on the device from the 64-byte per-UE log records a simulation kernel writes there
// (prach_ue_log: words 1-3 timer, active, txTime; word 14 msg4Flag) and from the trial's arrival schedule, which the launch has on the device
// anyway.  gfx950 only.  prach_timeline_accumulate_logs (prach_host.c) is the definition; this kernel equals it integer for integer.
//
// The engine launches it on its stream behind a simulation launch, for the trials whose result it keeps.  A workgroup takes ONE tile of TL_TILE
// consecutive UEs of ONE trial (the job table gives every trial its first workgroup).  UEs are activated in index order, so the arrival slots of
// a tile are one contiguous range of the schedule (tile_slots of prach_reduce_tile.h, which also has the job lookup, the wavefront folds and the
// flush of the scalars that the reducer kernels share).
//
// SCHEME 1 privatises TL_WINDOW bins, anchored at the tile's first arrival bin, in LDS: four 32-bit counters per by-arrival bin (arrivals,
// success, sojourn sum, timer sum: a tile's sums fit 32 bits, prach_device.h) and one per done bin.  Only non-zero bins are flushed, with
// 64-bit agent-scope atomic adds (trials of one group run on different XCDs).  What falls outside a window goes straight to the global bins
// with the same atomics, and so does everything under SCHEME 0.  The scalars are reduced per wavefront.  Integers only: the result does not
// depend on any order.  Engine option "timeline_scheme"; DESIGN.md 4 has the measurements.
#include "prach_reduce_tile.h"

namespace prach {

namespace {

template <int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void timeline_kernel(const TimelineJob *__restrict__ jobs, int njobs, int bins, int width, TimelineOut out) {
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | 8 x 64-bit scalars | SCHEME 1: [TL_WINDOW][4] by-arrival | [TL_WINDOW] done
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const lwin = lds + TILE_SCHED_CAP + 2 * TL_SCALARS;
    unsigned *const ldone = lwin + 4 * TL_WINDOW;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);

    // the tile's slot range (the same in every thread) and its first arrival bin: the anchor of both windows
    const TileSlots S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    const unsigned bin0 = (unsigned)(J.aT * S.slo) / (unsigned)width;
    if (SCHEME == 1)
        for (int b = tid; b < 5 * TL_WINDOW; b += TL_THREADS) lwin[b] = 0;
    if (tid < TL_SCALARS) lsc[tid] = 0;
    __syncthreads();

    unsigned long long *const g_arr = out.arrivals + (size_t)J.group * (size_t)bins, *const g_suc = out.success + (size_t)J.group * (size_t)bins,
                       *const g_soj = out.sojourn + (size_t)J.group * (size_t)bins, *const g_tim = out.timer + (size_t)J.group * (size_t)bins,
                       *const g_don = out.done + (size_t)J.group * (size_t)bins;
    unsigned arrived = 0, nsucc = 0, nrest = 0, aover = 0, dover = 0, dmax1 = 0;
    unsigned long long ssum = 0, tsum = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const int4 head = J.logs[4 * (size_t)i]; // idx, timer, active, txTime
        if (head.z == -1) continue;              // not arrived
        const bool ok = J.logs[4 * (size_t)i + 3].z == 1; // msg4Flag
        const unsigned a = (unsigned)S.arrival(J, i);
        const unsigned ab = width == 1 ? a : a / (unsigned)width;
        const bool abin = ab < (unsigned)bins, awin = SCHEME == 1 && abin && ab - bin0 < (unsigned)TL_WINDOW;
        arrived++;
        if (!abin) aover++;
        else if (awin) atomicAdd(&lwin[4 * (ab - bin0)], 1u);
        else agent_add(&g_arr[ab], 1ull);
        if (!ok) continue;
        const unsigned timer = (unsigned)head.y, c = (unsigned)(head.w + 6), soj = c - a;
        const unsigned db = width == 1 ? c : c / (unsigned)width;
        nsucc++;
        nrest += c - timer != a;
        ssum += soj;
        tsum += timer;
        dmax1 = max(dmax1, c + 1u);
        // (a sum past the 32-bit budget of a tile cannot come from a simulation kernel, whose timer never exceeds the sojourn; the definition takes any
        // timer >= 0, so both addends are held to the budget and a larger one goes the exact way)
        if (awin && soj <= (unsigned)TL_MAX_SOJOURN && timer <= (unsigned)TL_MAX_SOJOURN) {
            atomicAdd(&lwin[4 * (ab - bin0) + 1], 1u);
            atomicAdd(&lwin[4 * (ab - bin0) + 2], soj);
            atomicAdd(&lwin[4 * (ab - bin0) + 3], timer);
        } else if (abin) {
            agent_add(&g_suc[ab], 1ull);
            agent_add(&g_soj[ab], (unsigned long long)soj);
            agent_add(&g_tim[ab], (unsigned long long)timer);
        }
        if (db >= (unsigned)bins) dover++;
        else if (SCHEME == 1 && db - bin0 < (unsigned)TL_WINDOW) atomicAdd(&ldone[db - bin0], 1u);
        else agent_add(&g_don[db], 1ull);
    }
    arrived = fold_sum(arrived); nsucc = fold_sum(nsucc); nrest = fold_sum(nrest); aover = fold_sum(aover); dover = fold_sum(dover);
    ssum = fold_sum(ssum); tsum = fold_sum(tsum); dmax1 = fold_max(dmax1);
    if (lane == 0 && arrived) {
        atomicAdd(&lsc[0], (unsigned long long)arrived); atomicAdd(&lsc[1], (unsigned long long)nsucc); atomicAdd(&lsc[2], (unsigned long long)nrest);
        atomicAdd(&lsc[3], (unsigned long long)aover); atomicAdd(&lsc[4], (unsigned long long)dover); atomicAdd(&lsc[5], ssum); atomicAdd(&lsc[6], tsum);
        atomicMax(&lsc[7], (unsigned long long)dmax1);
    }
    __syncthreads();

    // flush: only what this tile touched (a window bin that was added to lies below `bins`)
    if (SCHEME == 1) {
        for (int b = tid; b < TL_WINDOW; b += TL_THREADS) {
            const uint4 v = *reinterpret_cast<const uint4 *>(&lwin[4 * b]);
            const size_t at = (size_t)bin0 + (size_t)b;
            if (v.x) agent_add(&g_arr[at], (unsigned long long)v.x);
            if (v.y) agent_add(&g_suc[at], (unsigned long long)v.y);
            if (v.z) agent_add(&g_soj[at], (unsigned long long)v.z);
            if (v.w) agent_add(&g_tim[at], (unsigned long long)v.w);
            const unsigned dn = ldone[b];
            if (dn) agent_add(&g_don[at], (unsigned long long)dn);
        }
    }
    flush_scalars(lsc, out.scalars + (size_t)J.group * TL_SCALARS, TL_SUMS, TL_MAXIMA, tid);
}

size_t timeline_lds_bytes(int scheme) { return 4 * (size_t)(TILE_SCHED_CAP + 2 * TL_SCALARS + (scheme == 1 ? 5 * TL_WINDOW : 0)); }

} // namespace

hipError_t launch_timeline_kernel(const TimelineJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, TimelineOut out, hipStream_t stream) {
    const size_t lds = timeline_lds_bytes(scheme);
    if (scheme == 0) return launch_with_lds(timeline_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, bins, bin_ms, out);
    return launch_with_lds(timeline_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, bins, bin_ms, out);
}

} // namespace prach
