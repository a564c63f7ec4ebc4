// prach_xtab.hip — prach::xtab_kernel: per trial group, a two-axis cross-tabulation over the fixed menu of per-UE quantities of include/prach.h
// (prach_run_trials_xtab), with a choice of which classes of UEs enter, reduced on the device from the 64-byte per-UE log records a simulation kernel
// writes there, the trial's arrival schedule and its `steps`.  gfx950 only.  prach_xtab_accumulate_logs (prach_host.c) is the definition; this kernel
// equals it integer for integer.
//
// Shape and jobs are prach_reduce_tile.h's, as prach::timeline_kernel's are: a workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial; where an
// axis needs a(i), and only there, the tile's slot range and every UE's arrival come from tile_slots.  TimelineJob::pad carries E = min(steps, maxTime)
// for this kind.
//
// A lane always reads words 0-3 (timer, active, txTime) and 12-15 (connectionRequest, msg4Flag, failCount) of a record; words 4-7 (nowBackoff) only
// when an axis is STATE and words 8-11 (preambleTxCounter) only when an axis is PTC: both uniform for the launch, so a launch moves 32-64 B per UE.
//
// TWO PATHS, by the size of the table, (row_bins + 1) x (col_bins + 1) cells:
//   1  at most XT_WINDOW_WORDS cells, SCHEME 1: the WHOLE table is privatised in LDS as 32-bit cells (a tile adds at most TL_TILE to one:
//      prach_device.h).  The dynamic LDS is sized by the table, not by the cap, so a small table leaves several workgroups per CU.  The table is zeroed
//      and scanned once; non-zero cells are flushed with 64-bit agent-scope atomic adds (trials of one group run on different XCDs).  A table of at most
//      XT_COPY_WORDS / 4 cells is kept in one copy per wavefront (with STATE or ONE on an axis most lanes of a wavefront hit one to three addresses);
//      the flush adds the copies up.
//   2  a larger table, and everything under SCHEME 0: every contribution goes straight to its global cell with the same atomics.
// The arrival-anchored row window of prach::sojourn_kernel is NOT rebuilt here: a fine ARRIVAL x SOJOURN table remains prach_run_trials_sojourn's job.
// The scalars are reduced per wavefront.  Integers only: the result does not depend on any order.  Engine option "xtab_scheme".
#include "prach_reduce_tile.h"
#include "prach_xtab_menu.h"

namespace prach {

namespace {

#ifndef PRACH_XT_COPY_WORDS
#define PRACH_XT_COPY_WORDS 4096 // (a build with 0 keeps one copy always: the measurement of DESIGN.md 4)
#endif
constexpr int XT_COPY_WORDS = PRACH_XT_COPY_WORDS; // LDS words that the per-wavefront copies of a table take at most
constexpr int XT_WAVES = TL_THREADS / 64;
static_assert(4 * (TILE_SCHED_CAP + 2 * XT_SCALARS + XT_WINDOW_WORDS) <= 160 * 1024 && XT_COPY_WORDS <= XT_WINDOW_WORDS,
              "the largest layout (a table of XT_WINDOW_WORDS cells) fits the 160 KiB of LDS of a gfx950 CU");

template <int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void xtab_kernel(const TimelineJob *__restrict__ jobs, int njobs, XtabAxes ax, int copies, XtabOut out) {
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | XT_SCALARS x 64-bit scalars | path 1: [copies][ncell] cells
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const lcell = lds + TILE_SCHED_CAP + 2 * XT_SCALARS;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    const unsigned W = (unsigned)ax.col_bins + 1u, ncell = ((unsigned)ax.row_bins + 1u) * W; // (the engine refuses a table of more than 2^27 cells)
    const bool priv = SCHEME == 1 && ncell <= (unsigned)XT_WINDOW_WORDS;                      // path 1
    const bool need_a = needs_arrival(ax.row_field) || needs_arrival(ax.col_field);
    const bool need_b = ax.row_field == PRACH_XTAB_STATE || ax.col_field == PRACH_XTAB_STATE;
    const bool need_p = ax.row_field == PRACH_XTAB_PTC || ax.col_field == PRACH_XTAB_PTC;

    // the tile's slot range, only where an axis needs it: no search and no copy otherwise
    TileSlots S{0, 0, J.sched, 0};
    if (need_a) S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (priv)
        for (unsigned w = tid; w < ncell * (unsigned)copies; w += TL_THREADS) lcell[w] = 0;
    if (tid < XT_SCALARS) lsc[tid] = 0;
    __syncthreads();

    unsigned long long *const g_cell = out.cells + (size_t)J.group * (size_t)ncell;
    unsigned *const mycell = lcell + (copies > 1 ? (unsigned)(tid >> 6) * ncell : 0u);
    unsigned nidle = 0, nserved = 0, nunserved = 0, nsel = 0, nbinned = 0;
    unsigned long long rsum = 0, csum = 0, rmax1 = 0, cmax1 = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const int4 head = J.logs[4 * (size_t)i];     // idx, timer, active, txTime
        const int4 tail = J.logs[4 * (size_t)i + 3]; // msg2Flag, connectionRequest, msg4Flag, failCount
        const int nowBackoff = need_b ? J.logs[4 * (size_t)i + 1].z : 0;
        const int ptc = need_p ? J.logs[4 * (size_t)i + 2].w : 0;
        const int cls = head.z == -1 ? 0 : tail.z == 1 ? 1 : 2;
        nidle += cls == 0; nserved += cls == 1; nunserved += cls == 2;
        const int bit = cls == 0 ? PRACH_XTAB_IDLE : cls == 1 ? PRACH_XTAB_SERVED : PRACH_XTAB_UNSERVED;
        if (!(ax.who & bit)) continue;
        nsel++;
        const int a = need_a ? S.arrival(J, i) : 0;
        const long long rv = xt_value(ax.row_field, head, tail, nowBackoff, ptc, cls, a, E), cv = xt_value(ax.col_field, head, tail, nowBackoff, ptc, cls, a, E);
        if (rv < 0 || cv < 0) continue; // UNDEFINED
        // (a value is below 2^31 + 6: it fits 32 unsigned bits, and the quotient is cut at the overflow bin)
        const unsigned r = min((unsigned)rv / (unsigned)ax.row_width, (unsigned)ax.row_bins), c = min((unsigned)cv / (unsigned)ax.col_width, (unsigned)ax.col_bins);
        const unsigned cell = r * W + c;
        nbinned++;
        rsum += (unsigned long long)rv; csum += (unsigned long long)cv;
        rmax1 = max(rmax1, (unsigned long long)rv + 1ull); cmax1 = max(cmax1, (unsigned long long)cv + 1ull);
        if (priv) atomicAdd(&mycell[cell], 1u);
        else agent_add(&g_cell[cell], 1ull);
    }
    nidle = fold_sum(nidle); nserved = fold_sum(nserved); nunserved = fold_sum(nunserved); nsel = fold_sum(nsel); nbinned = fold_sum(nbinned);
    rsum = fold_sum(rsum); csum = fold_sum(csum); rmax1 = fold_max(rmax1); cmax1 = fold_max(cmax1);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)nidle); atomicAdd(&lsc[1], (unsigned long long)nserved); atomicAdd(&lsc[2], (unsigned long long)nunserved);
        atomicAdd(&lsc[3], (unsigned long long)nsel); atomicAdd(&lsc[4], (unsigned long long)nbinned); atomicAdd(&lsc[5], rsum); atomicAdd(&lsc[6], csum);
        atomicMax(&lsc[7], rmax1); atomicMax(&lsc[8], cmax1);
    }
    __syncthreads();

    // flush: only what this tile touched
    if (priv)
        for (unsigned w = tid; w < ncell; w += TL_THREADS) {
            unsigned v = lcell[w];
            for (int k = 1; k < copies; k++) v += lcell[(unsigned)k * ncell + w];
            if (v) agent_add(&g_cell[w], (unsigned long long)v);
        }
    flush_scalars(lsc, out.scalars + (size_t)J.group * XT_SCALARS, XT_SUMS, XT_MAXIMA, tid);
}

} // namespace

hipError_t launch_xtab_kernel(const TimelineJob *jobs, int njobs, int workgroups, XtabAxes ax, int scheme, XtabOut out, hipStream_t stream) {
    const size_t ncell = ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const bool priv = scheme == 1 && ncell <= (size_t)XT_WINDOW_WORDS;
    const int copies = priv && ncell * XT_WAVES <= (size_t)XT_COPY_WORDS ? XT_WAVES : 1;
    const size_t lds = 4 * ((size_t)TILE_SCHED_CAP + 2 * XT_SCALARS + (priv ? ncell * (size_t)copies : 0));
    if (scheme == 0) return launch_with_lds(xtab_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, ax, copies, out);
    return launch_with_lds(xtab_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, ax, copies, out);
}

} // namespace prach
