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
#include "prach_reduce_tile.h"
#include "prach_xtab_menu.h"

namespace prach {

namespace {

// word w (0 .. 15) of a record from its four quarters; w is uniform
__device__ __forceinline__ int record_word(int w, const int4 &q0, const int4 &q1, const int4 &q2, const int4 &q3) {
    const int4 q = (w >> 2) == 0 ? q0 : (w >> 2) == 1 ? q1 : (w >> 2) == 2 ? q2 : q3;
    return (w & 3) == 0 ? q.x : (w & 3) == 1 ? q.y : (w & 3) == 2 ? q.z : q.w;
}

__global__ __launch_bounds__(TL_THREADS) void columns_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_columns_spec sp, ColumnsOut out) {
    __shared__ int lsched[TILE_SCHED_CAP];
    __shared__ unsigned long long lsc[CL_SCALARS];
    const int tid = threadIdx.x, lane = tid & 63;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;

    // what the columns need, as 0 / 1
    int need_a = 0, need_q1 = 0, need_q2 = 0;
    for (int c = 0; c < sp.ncols; c++) {
        const int f = sp.field[c], w = f - PRACH_COL_RAW;
        need_a |= (int)needs_arrival(f);
        need_q1 |= (int)(f == PRACH_XTAB_STATE) | (int)((w >> 2) == 1);
        need_q2 |= (int)(f == PRACH_XTAB_PTC) | (int)((w >> 2) == 2);
    }

    // the tile's slot range, only where a column needs it: no search and no copy otherwise
    TileSlots S{0, 0, J.sched, 0};
    if (need_a) S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (tid < CL_SCALARS) lsc[tid] = 0;
    __syncthreads();

    int *const col0 = out.data + out.offset[J.group]; // the trial's segment of column 0
    unsigned nidle = 0, nserved = 0, nunserved = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const int4 head = J.logs[4 * (size_t)i];     // idx, timer, active, txTime
        const int4 tail = J.logs[4 * (size_t)i + 3]; // msg2Flag, connectionRequest, msg4Flag, failCount
        int4 q1 = make_int4(0, 0, 0, 0), q2 = make_int4(0, 0, 0, 0);
        if (need_q1) q1 = J.logs[4 * (size_t)i + 1]; // firstTxTime, secondTxTime, nowBackoff, preamble
        if (need_q2) q2 = J.logs[4 * (size_t)i + 2]; // preambleChange, rarWindow, maxRarCounter, preambleTxCounter
        const int cls = head.z == -1 ? 0 : tail.z == 1 ? 1 : 2;
        nidle += cls == 0; nserved += cls == 1; nunserved += cls == 2;
        const int a = need_a ? S.arrival(J, i) : 0;
        for (int c = 0; c < sp.ncols; c++) {
            const int f = sp.field[c];
            int v;
            if (f >= PRACH_COL_RAW) v = record_word(f - PRACH_COL_RAW, head, q1, q2, tail);
            else {
                const long long x = xt_value(f, head, tail, q1.z, q2.w, cls, a, E);
                v = x < 0 ? -1 : (int)x;
            }
            col0[(size_t)c * out.stride + (size_t)i] = v;
        }
    }
    nidle = fold_sum(nidle); nserved = fold_sum(nserved); nunserved = fold_sum(nunserved);
    if (lane == 0) { atomicAdd(&lsc[0], (unsigned long long)nidle); atomicAdd(&lsc[1], (unsigned long long)nserved); atomicAdd(&lsc[2], (unsigned long long)nunserved); }
    __syncthreads();
    flush_scalars(lsc, out.scalars + (size_t)J.group * CL_SCALARS, CL_SUMS, 0, tid);
}

} // namespace

hipError_t launch_columns_kernel(const TimelineJob *jobs, int njobs, int workgroups, const prach_columns_spec &spec, ColumnsOut out, hipStream_t stream) {
    if (!prach_internal_columns_spec_ok(&spec) || !out.data || !out.offset || !out.scalars) return hipErrorInvalidValue;
    hipLaunchKernelGGL(columns_kernel, dim3(workgroups), dim3(TL_THREADS), 0, stream, jobs, njobs, spec, out);
    return hipGetLastError();
}

} // namespace prach
