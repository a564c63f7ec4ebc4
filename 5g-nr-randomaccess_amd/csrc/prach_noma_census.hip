// prach_noma_census.hip — the two kernels over THE NOMA MENU of include/prach.h, reduced on the device from the 64-byte per-UE log records prach::noma_kernel
// writes there, the trial's arrival schedule and its `steps`.  gfx950 only.
//   prach::noma_census_kernel   per trial group a two-axis cross-tabulation with a choice of classes (prach_run_trials_noma_census);
//                               prach_noma_census_accumulate_logs (prach_host.c) is the definition
//   prach::noma_columns_kernel  per UE of every trial the asked-for fields and raw record words as int32 columns (prach_run_trials_noma_columns, _device);
//                               prach_noma_columns_from_logs is the definition
// Both equal their definition integer for integer.  They have the shape of prach::xtab_kernel and prach::columns_kernel and share everything those share
// (prach_reduce_tile.h: tile, jobs, slot range, folds, flush) AND their bodies: census_body and columns_body of prach_menu_body.h, instantiated here with
// NomaMenu (prach_noma_menu.h) and in prach_xtab.hip / prach_columns.hip with XtabMenu.  What differs between the menus — the record quarters a launch loads,
// the class and its four counters against three (one scalar more per group and per trial), the value — is the policy's; the table paths, the folds and the
// flush are written once.  The __global__ functions stay in this file under their own names and arguments, so the symbols that profiles, harnesses
// (tests/tools/gpu_noma_census_harness.hip includes this file) and the ISA inventory know are unchanged (profiles/menu_bodies.md).
//
// A workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial; TimelineJob::pad carries E = min(steps, maxTime).  A lane always reads words 8-11
// (preambleChange = the sector, maxRarCounter, preambleTxCounter) and 12-15 (connectionRequest, msg4Flag, failCount) of a record: the class needs them.
// Words 0-3 and 4-7 only where a field needs them (nm_needs_q0, nm_needs_q1): uniform for the launch, so a launch moves 32-64 B per UE.
//
// CENSUS, two paths by the size of the table, as in prach_xtab.hip: at most XT_WINDOW_WORDS cells under scheme 1 — the whole table privatised in LDS as
// 32-bit cells (a tile adds at most TL_TILE to one), one copy per wavefront while the copies fit NC_COPY_WORDS words (STATE, SECTOR or ONE on an axis puts a
// wavefront on one to nine addresses), non-zero cells flushed with 64-bit agent-scope atomic adds; a larger table, and everything under scheme 0, straight
// to its global cell with the same atomics.  The scalars are folded per wavefront.  Engine option "xtab_scheme".
// COLUMNS: one 4-byte store per lane and column, consecutive lanes at consecutive addresses; a trial's offset is any number of rows, so nothing is wider
// than a word.  Plain stores: a trial has a job only in the launch whose result is kept.
#include "prach_menu_body.h"
#include "prach_noma_menu.h"

namespace prach {

namespace {

constexpr int NC_COPY_WORDS = 4096; // LDS words that the per-wavefront copies of a table take at most (prach_xtab.hip's measured limit)
constexpr int NC_WAVES = TL_THREADS / 64;
static_assert(4 * (TILE_SCHED_CAP + 2 * NC_SCALARS + XT_WINDOW_WORDS) <= 160 * 1024 && NC_COPY_WORDS <= XT_WINDOW_WORDS,
              "the largest layout (a table of XT_WINDOW_WORDS cells) fits the 160 KiB of LDS of a gfx950 CU");
static_assert(CENSUS_SUMS<NomaMenu> == NC_SUMS && NC_SUMS + NC_MAXIMA <= NC_SCALARS && NomaMenu::NCLASSES == NCL_SUMS, "the bodies' scalar rows are the ones prach_device.h states");

template <int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void noma_census_kernel(const TimelineJob *__restrict__ jobs, int njobs, XtabAxes ax, int copies, XtabOut out) {
    census_body<NomaMenu, SCHEME>(jobs, njobs, ax, copies, out);
}

__global__ __launch_bounds__(TL_THREADS) void noma_columns_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_columns_spec sp, ColumnsOut out) {
    columns_body<NomaMenu>(jobs, njobs, sp, out);
}

} // namespace

hipError_t launch_noma_census_kernel(const TimelineJob *jobs, int njobs, int workgroups, XtabAxes ax, int scheme, XtabOut out, hipStream_t stream) {
    const size_t ncell = ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const bool priv = scheme == 1 && ncell <= (size_t)XT_WINDOW_WORDS;
    const int copies = priv && ncell * NC_WAVES <= (size_t)NC_COPY_WORDS ? NC_WAVES : 1;
    const size_t lds = 4 * ((size_t)TILE_SCHED_CAP + 2 * NC_SCALARS + (priv ? ncell * (size_t)copies : 0));
    if (scheme == 0) return launch_with_lds(noma_census_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, ax, copies, out);
    return launch_with_lds(noma_census_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, ax, copies, out);
}
int noma_census_copy_words() { return NC_COPY_WORDS; }

hipError_t launch_noma_columns_kernel(const TimelineJob *jobs, int njobs, int workgroups, const prach_columns_spec &spec, ColumnsOut out, hipStream_t stream) {
    if (!prach_internal_noma_columns_spec_ok(&spec) || !out.data || !out.offset || !out.scalars) return hipErrorInvalidValue;
    hipLaunchKernelGGL(noma_columns_kernel, dim3(workgroups), dim3(TL_THREADS), 0, stream, jobs, njobs, spec, out);
    return hipGetLastError();
}

} // namespace prach
