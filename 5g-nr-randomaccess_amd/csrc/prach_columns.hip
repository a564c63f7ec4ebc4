// prach_columns.hip — prach::columns_kernel: per UE of every trial (prach_run_trials_columns, prach_run_trials_columns_device) the asked-for fields of
// the menu of per-UE quantities of include/prach.h, and raw words of the 64-byte log record, as plain int32 COLUMNS, computed on the device from the log
// records a simulation kernel writes there, the trial's arrival schedule and its `steps`.  Nothing is reduced: the other kinds answer a fixed question,
// this one exports the values behind them, to the host or into device memory the caller owns.  gfx950 only.  prach_columns_from_logs (prach_host.c) is
// the definition; this kernel equals it integer for integer.
//
// Shape and jobs are prach_reduce_tile.h's, as prach::xtab_kernel's are: a workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial;
// TimelineJob::pad carries E = min(steps, maxTime) and `group` is the trial, whose first row comes from the call's offset table (one 64-bit word per
// trial, uploaded once per call behind the scalars).  Column c of UE i of trial k is the word out[c * stride + offset[k] + i].
//
// LOADS: a lane always reads words 0-3 (timer, active, txTime) and 12-15 (msg4Flag, failCount) of a record; words 4-7 only where a column is STATE or a
// raw word among them, words 8-11 only where one is PTC or a raw word among them; the tile's slot range and a(i) (tile_slots) only where a column needs
// a(i).  All of it, and the field of every column, is uniform for the launch: scalar branches.
// STORES: one 4-byte store per lane and column, consecutive lanes at consecutive addresses (256 B per wavefront-instruction).  A trial's offset is any
// number of rows, so a column segment is 4-byte aligned and nothing more: no store is wider than a word.  Plain stores, no atomics on the columns: a
// trial has a job only in the launch whose result is kept, so a word is written once.  The three class counts are folded per wavefront, added up in LDS
// and flushed with 64-bit agent-scope adds (the tiles of a trial run on different XCDs).
//
// THE BOUND: every menu value of a trial fits int32.  ARRIVAL, COMPLETION and AGE are subframe numbers of a trial of at most 60 000 + 6 subframes, SOJOURN is
// at most TL_MAX_SOJOURN, TIMER, PTC and FAILCOUNT are logged int32 words, STATE is at most 6; xt_value computes in 64 bits and the column takes the low
// word.  A NEGATIVE menu value is UNDEFINED (the one rule of the menu) and is stored as -1; a raw word is stored as it is.
// THE BODY is columns_body<XtabMenu> of prach_menu_body.h, shared with prach::noma_columns_kernel; the kernel's name, arguments and launch are here.
#include "prach_menu_body.h"
#include "prach_xtab_menu.h"

namespace prach {

namespace {

static_assert(XtabMenu::NCLASSES == CL_SUMS, "the body's scalar row is the one prach_device.h states");

__global__ __launch_bounds__(TL_THREADS) void columns_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_columns_spec sp, ColumnsOut out) {
    columns_body<XtabMenu>(jobs, njobs, sp, out);
}

} // namespace

hipError_t launch_columns_kernel(const TimelineJob *jobs, int njobs, int workgroups, const prach_columns_spec &spec, ColumnsOut out, hipStream_t stream) {
    if (!prach_internal_columns_spec_ok(&spec) || !out.data || !out.offset || !out.scalars) return hipErrorInvalidValue;
    hipLaunchKernelGGL(columns_kernel, dim3(workgroups), dim3(TL_THREADS), 0, stream, jobs, njobs, spec, out);
    return hipGetLastError();
}

} // namespace prach
