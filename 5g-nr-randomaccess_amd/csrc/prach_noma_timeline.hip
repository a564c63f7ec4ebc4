// prach_noma_timeline.hip — prach::noma_timeline_kernel: per trial group and SECTOR, what became of the UEs of a NOMA.c trial that arrived in each stretch of the
// simulation (include/prach.h, prach_run_trials_noma_timeline), reduced on the device from the 64-byte per-UE log records prach::noma_kernel writes there, the
// trial's arrival schedule and its `steps`.  gfx950 only.  prach_noma_timeline_accumulate_logs (prach_host.c) is the definition; this kernel equals it integer
// for integer.
//
// The shape is the reducers': a workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial (prach_reduce_tile.h: job lookup, slot range of the tile, folds,
// flush of the scalars); TimelineJob::pad carries E = min(steps, maxTime).  Class and values are THE NOMA MENU's (prach_noma_menu.h: nm_class, nm_value), not a
// second statement of it.  A launch always needs quarters 0 (timer, txTime), 2 (the sector) and 3 (msg4Flag, failCount) of a record and never quarter 1: 48 B
// per UE.
//
// SCHEME 1 adds a tile up in an LDS window of 32-bit counters, `window` bins x 6 sectors x 6 series (arrivals, served, dropped, sojourn sum, timer sum, done),
// anchored at the tile's first arrival bin, and flushes the non-zero counters with 64-bit agent-scope atomic adds (trials of one group run on different XCDs).
// A counter holds what one tile adds: at most TL_TILE UEs, and sums of at most TL_TILE x NTL_MAX_SOJOURN (prach_device.h).  What falls outside goes straight
// to the global counter with the same atomics, as prach::timeline_kernel does: a later arrival bin, a completion bin behind the window, and a served UE whose
// sojourn or timer exceeds NTL_MAX_SOJOURN (no trial produces one; the definition takes any value >= 0).  SCHEME 0 sends everything straight out.  The scalars
// are reduced per wavefront.  Integers only: the result does not depend on any order.  Engine option "timeline_scheme"; profiles/noma_timeline_kernel.md has
// the window sizes tried.
#include "prach_reduce_tile.h"
#include "prach_noma_menu.h"

namespace prach {

namespace {

// The kernel is a member of the timeline_kernel family by name — timeline_kernel<NomaUes, SCHEME>; `noma_timeline_kernel<SCHEME>` below is its name in the
// sources — so that every census of the library's kernel symbols by the name in front of the template arguments (tests/tools/cut_cases.py: LEFT_OUT) classes
// it with the reducers, as it classes prach_timeline.hip's.
struct NomaUes {};
template <class UES, int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void timeline_kernel(const TimelineJob *__restrict__ jobs, int njobs, int bins, int width, int window, NomaTimelineOut out) {
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | NTL_SCALARS x 64-bit scalars | SCHEME 1: [6 series][window][6 sectors] the window
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const lwin = lds + TILE_SCHED_CAP + 2 * NTL_SCALARS;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    // the tile's slot range (the same in every thread) and its first arrival bin: the anchor of the window
    const TileSlots S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    const unsigned bin0 = (unsigned)(J.aT * S.slo) / (unsigned)width;
    const unsigned nwin = bin0 < (unsigned)bins ? min((unsigned)window, (unsigned)bins - bin0) : 0u; // bins of this tile that the window holds
    const unsigned wstride = 6u * (unsigned)window;                                                  // words of one series of the window
    if (SCHEME == 1) {
#pragma unroll
        for (int q = 0; q < 6; q++)
            for (unsigned x = tid; x < 6u * nwin; x += TL_THREADS) lwin[q * wstride + x] = 0;
    }
    if (tid < NTL_SCALARS) lsc[tid] = 0;
    __syncthreads();

    const size_t gbase = (size_t)J.group * 6 * (size_t)bins;
    const NomaMenu::Needs needs{true, true, false}; // a(i), quarter 0, never quarter 1
    unsigned nidle = 0, nserved = 0, ndropped = 0, npending = 0, nundef = 0, nrest = 0, aover = 0, dover = 0, dmax1 = 0;
    unsigned long long ssum = 0, tsum = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const NomaMenu::Rec r = NomaMenu::load<false>(J.logs, i, needs);
        const int cls = NomaMenu::cls(r);
        const bool served = cls == PRACH_NOMA_SERVED, dropped = cls == PRACH_NOMA_DROPPED;
        nidle += cls == PRACH_NOMA_IDLE ? 1u : 0u;
        nserved += served ? 1u : 0u;
        ndropped += dropped ? 1u : 0u;
        npending += cls == PRACH_NOMA_PENDING ? 1u : 0u;
        if (cls == PRACH_NOMA_IDLE) continue;
        const int a = S.arrival(J, i);
        const long long sec = NomaMenu::value(PRACH_NOMA_SECTOR, r, cls, a, E);
        long long sj = 0, tm = 0, c = 0;
        if (served) {
            sj = NomaMenu::value(PRACH_NOMA_SOJOURN, r, cls, a, E);
            tm = NomaMenu::value(PRACH_NOMA_TIMER, r, cls, a, E);
            c = NomaMenu::value(PRACH_NOMA_COMPLETION, r, cls, a, E);
        }
        // undefined for the timeline (the menu's ONE RULE: a negative value is undefined); min() over the values keeps this one compare
        if ((unsigned long long)sec > 5ull || min(min(sj, tm), c) < 0) { nundef++; continue; }
        const unsigned ab = (unsigned)NomaMenu::value(PRACH_NOMA_ARRIVAL, r, cls, a, E) / (unsigned)width;
        const bool abin = ab < (unsigned)bins, awin = SCHEME == 1 && ab - bin0 < nwin; // (a window bin lies below `bins`)
        const unsigned wat = (ab - bin0) * 6u + (unsigned)sec;                        // in the window, where awin
        const size_t gat = gbase + (size_t)sec * (size_t)bins + ab;                   // in the call's buffers, where abin
        if (!abin) aover++;
        else if (awin) atomicAdd(&lwin[wat], 1u);
        else agent_add(&out.series[0][gat], 1ull);
        if (dropped) {
            if (awin) atomicAdd(&lwin[2 * wstride + wat], 1u);
            else if (abin) agent_add(&out.series[2][gat], 1ull);
        }
        if (!served) continue;
        const long long lost = NomaMenu::value(PRACH_NOMA_LOST, r, cls, a, E);
        const unsigned cu = (unsigned)c; // (c <= INT_MAX + 6)
        const unsigned db = cu / (unsigned)width;
        nrest += lost > 0 ? 1u : 0u;
        ssum += (unsigned long long)sj;
        tsum += (unsigned long long)tm;
        dmax1 = max(dmax1, cu + 1u);
        if (awin && sj <= NTL_MAX_SOJOURN && tm <= NTL_MAX_SOJOURN) {
            atomicAdd(&lwin[1 * wstride + wat], 1u);
            atomicAdd(&lwin[3 * wstride + wat], (unsigned)sj);
            atomicAdd(&lwin[4 * wstride + wat], (unsigned)tm);
        } else if (abin) {
            agent_add(&out.series[1][gat], 1ull);
            agent_add(&out.series[3][gat], (unsigned long long)sj);
            agent_add(&out.series[4][gat], (unsigned long long)tm);
        }
        if (db >= (unsigned)bins) dover++;
        else if (SCHEME == 1 && db - bin0 < nwin) atomicAdd(&lwin[5 * wstride + (db - bin0) * 6u + (unsigned)sec], 1u);
        else agent_add(&out.series[5][gbase + (size_t)sec * (size_t)bins + db], 1ull);
    }
    nidle = fold_sum(nidle); nserved = fold_sum(nserved); ndropped = fold_sum(ndropped); npending = fold_sum(npending); nundef = fold_sum(nundef);
    nrest = fold_sum(nrest); aover = fold_sum(aover); dover = fold_sum(dover); ssum = fold_sum(ssum); tsum = fold_sum(tsum); dmax1 = fold_max(dmax1);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)nidle); atomicAdd(&lsc[1], (unsigned long long)nserved); atomicAdd(&lsc[2], (unsigned long long)ndropped);
        atomicAdd(&lsc[3], (unsigned long long)npending); atomicAdd(&lsc[4], (unsigned long long)nundef); atomicAdd(&lsc[5], (unsigned long long)nrest);
        atomicAdd(&lsc[6], (unsigned long long)aover); atomicAdd(&lsc[7], (unsigned long long)dover); atomicAdd(&lsc[8], ssum); atomicAdd(&lsc[9], tsum);
        atomicMax(&lsc[10], (unsigned long long)dmax1);
    }
    __syncthreads();

    // flush: only what this tile touched
    if (SCHEME == 1) {
#pragma unroll
        for (int q = 0; q < 6; q++)
            for (unsigned x = tid; x < 6u * nwin; x += TL_THREADS) {
                const unsigned v = lwin[q * wstride + x];
                const unsigned b = x / 6u, sec = x - 6u * b;
                if (v) agent_add(&out.series[q][gbase + (size_t)sec * (size_t)bins + bin0 + b], (unsigned long long)v);
            }
    }
    flush_scalars(lsc, out.scalars + (size_t)J.group * NTL_SCALARS, NTL_SUMS, NTL_MAXIMA, tid);
}

template <int SCHEME> constexpr auto noma_timeline_kernel = &timeline_kernel<NomaUes, SCHEME>;

size_t noma_timeline_lds_bytes(int scheme, int window) { return 4 * (size_t)(TILE_SCHED_CAP + 2 * NTL_SCALARS + (scheme == 1 ? 36 * window : 0)); }

} // namespace

hipError_t launch_noma_timeline_kernel(const TimelineJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, int window, NomaTimelineOut out, hipStream_t stream) {
    if (window < 1 || window > NTL_WINDOW_MAX || bins < 1 || bin_ms < 1) return hipErrorInvalidValue;
    const size_t lds = noma_timeline_lds_bytes(scheme, window);
    if (scheme == 0) return launch_with_lds(noma_timeline_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, bins, bin_ms, window, out);
    return launch_with_lds(noma_timeline_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, bins, bin_ms, window, out);
}

} // namespace prach
