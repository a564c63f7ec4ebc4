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
// THE BODY is census_body<XtabMenu, SCHEME> of prach_menu_body.h, shared with prach::noma_census_kernel; the kernel's name, arguments and launch are here.
#include "prach_menu_body.h"
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
static_assert(CENSUS_SUMS<XtabMenu> == XT_SUMS && XT_SUMS + XT_MAXIMA <= XT_SCALARS, "the body's scalar row is the one prach_device.h states");

template <int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void xtab_kernel(const TimelineJob *__restrict__ jobs, int njobs, XtabAxes ax, int copies, XtabOut out) {
    census_body<XtabMenu, SCHEME>(jobs, njobs, ax, copies, out);
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
