// prach_sojourn.hip — prach::sojourn_kernel: per trial group, the histogram of the time from a UE's arrival to its Msg4 (the sojourn c(i) - a(i) of
// include/prach.h) by arrival row (prach_run_trials_sojourn), reduced on the device from the 64-byte per-UE log records a simulation kernel writes there
// (words 1-3 timer, active, txTime; word 14 msg4Flag) and from the trial's arrival schedule.  gfx950 only.  prach_sojourn_accumulate_logs
// (prach_host.c) is the definition; this kernel equals it integer for integer.
//
// Shape and jobs are prach_reduce_tile.h's, as prach::timeline_kernel's are: a workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial, and the
// tile's slot range and every UE's arrival come from tile_slots.
//
// UEs are activated in index order, so a tile's arrival rows are one contiguous range from row0 = a(first UE of the tile) / row_ms on.  SCHEME 1
// privatises its first R = min(rows - row0, SJ_WINDOW_WORDS / delay_bins) rows in LDS: R x delay_bins 32-bit cells (a tile adds at most TL_TILE to
// one: prach_device.h) and one arrived and one overflow counter per row.  Only the R x delay_bins words in use are zeroed and scanned; only non-zero
// counters are flushed, with 64-bit agent-scope atomic adds (trials of one group run on different XCDs).  What falls outside the window goes straight
// to the global cell with the same atomics (R may be 0: everything does), and so does everything under SCHEME 0.  The scalars are reduced per
// wavefront.  Integers only: the result does not depend on any order.  Engine option "sojourn_scheme".
#include "prach_reduce_tile.h"

namespace prach {

namespace {

static_assert(4 * (TILE_SCHED_CAP + 2 * SJ_SCALARS + 2 * PRACH_SOJOURN_MAX_ARRIVAL_BINS + SJ_WINDOW_WORDS) <= 160 * 1024,
              "the largest layout (every row privatised: the two per-row arrays at their longest next to a full window) fits the 160 KiB of LDS of a gfx950 CU");

// rows a workgroup can privatise at most: the launch sizes the two per-row counter arrays by it
int window_rows(int rows, int delay_bins) { return rows < SJ_WINDOW_WORDS / delay_bins ? rows : SJ_WINDOW_WORDS / delay_bins; }

template <int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void sojourn_kernel(const TimelineJob *__restrict__ jobs, int njobs, int rows, int row_ms, int dbins, int dwidth, int rcap,
                                                             SojournOut out) {
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | 8 x 64-bit scalars | SCHEME 1: [rcap] arrived | [rcap] overflow | [rcap x dbins] cells
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const larr = lds + TILE_SCHED_CAP + 2 * SJ_SCALARS;
    unsigned *const lovf = larr + rcap;
    unsigned *const lcell = lovf + rcap;

    const TimelineJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);

    // the tile's slot range (the same in every thread), its first arrival row and the rows of its window: row0 + R <= rows, R <= rcap
    const TileSlots S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    const unsigned row0 = (unsigned)(J.aT * S.slo) / (unsigned)row_ms;
    unsigned R = 0;
    if (SCHEME == 1) {
        if (row0 < (unsigned)rows) R = min((unsigned)rows - row0, (unsigned)rcap);
    }
    const unsigned ncell = R * (unsigned)dbins; // <= SJ_WINDOW_WORDS
    if (SCHEME == 1) {
        for (unsigned w = tid; w < ncell; w += TL_THREADS) lcell[w] = 0;
        for (unsigned r = tid; r < R; r += TL_THREADS) { larr[r] = 0; lovf[r] = 0; }
    }
    if (tid < SJ_SCALARS) lsc[tid] = 0;
    __syncthreads();

    unsigned long long *const g_cell = out.hist + (size_t)J.group * (size_t)rows * (size_t)dbins, *const g_arr = out.row_arrived + (size_t)J.group * (size_t)rows,
                       *const g_ovf = out.row_overflow + (size_t)J.group * (size_t)rows;
    unsigned arrived = 0, nsucc = 0, nrest = 0, aover = 0, dover = 0, smax1 = 0;
    unsigned long long ssum = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const int4 head = J.logs[4 * (size_t)i]; // idx, timer, active, txTime
        if (head.z == -1) continue;              // not arrived
        const bool ok = J.logs[4 * (size_t)i + 3].z == 1; // msg4Flag
        const unsigned a = (unsigned)S.arrival(J, i);
        const unsigned r = a / (unsigned)row_ms, wr = r - row0; // (r >= row0: arrivals follow the index)
        arrived++;
        if (r >= (unsigned)rows) aover++;
        else if (wr < R) atomicAdd(&larr[wr], 1u);
        else agent_add(&g_arr[r], 1ull);
        if (!ok) continue;
        const unsigned c = (unsigned)(head.w + 6), soj = c - a;
        const unsigned d = dwidth == 1 ? soj : soj / (unsigned)dwidth;
        nsucc++;
        nrest += c - (unsigned)head.y != a;
        ssum += soj;
        smax1 = max(smax1, soj + 1u);
        if (d >= (unsigned)dbins) dover++; // (the scalar counts every successful UE, in a row or not)
        if (r >= (unsigned)rows) continue;
        if (d < (unsigned)dbins) {
            if (wr < R) atomicAdd(&lcell[wr * (unsigned)dbins + d], 1u);
            else agent_add(&g_cell[(size_t)r * (size_t)dbins + d], 1ull);
        } else {
            if (wr < R) atomicAdd(&lovf[wr], 1u);
            else agent_add(&g_ovf[r], 1ull);
        }
    }
    arrived = fold_sum(arrived); nsucc = fold_sum(nsucc); nrest = fold_sum(nrest); aover = fold_sum(aover); dover = fold_sum(dover);
    ssum = fold_sum(ssum); smax1 = fold_max(smax1);
    if (lane == 0 && arrived) {
        atomicAdd(&lsc[0], (unsigned long long)arrived); atomicAdd(&lsc[1], (unsigned long long)nsucc); atomicAdd(&lsc[2], (unsigned long long)nrest);
        atomicAdd(&lsc[3], (unsigned long long)aover); atomicAdd(&lsc[4], (unsigned long long)dover); atomicAdd(&lsc[5], ssum);
        atomicMax(&lsc[6], (unsigned long long)smax1);
    }
    __syncthreads();

    // flush: only what this tile touched.  The window's rows are consecutive, so its cells are one run of the group's histogram from row0 on
    if (SCHEME == 1) {
        unsigned long long *const g_win = g_cell + (size_t)row0 * (size_t)dbins;
        for (unsigned w = tid; w < ncell; w += TL_THREADS) {
            const unsigned v = lcell[w];
            if (v) agent_add(&g_win[w], (unsigned long long)v);
        }
        for (unsigned r = tid; r < R; r += TL_THREADS) {
            const unsigned va = larr[r], vo = lovf[r];
            if (va) agent_add(&g_arr[row0 + r], (unsigned long long)va);
            if (vo) agent_add(&g_ovf[row0 + r], (unsigned long long)vo);
        }
    }
    flush_scalars(lsc, out.scalars + (size_t)J.group * SJ_SCALARS, SJ_SUMS, SJ_MAXIMA, tid);
}

} // namespace

hipError_t launch_sojourn_kernel(const TimelineJob *jobs, int njobs, int workgroups, int rows, int row_ms, int delay_bins, int delay_bin_ms, int scheme, SojournOut out,
                                 hipStream_t stream) {
    const int rcap = scheme == 1 ? window_rows(rows, delay_bins) : 0;
    const size_t lds = 4 * ((size_t)TILE_SCHED_CAP + 2 * SJ_SCALARS + 2 * (size_t)rcap + (size_t)rcap * (size_t)delay_bins);
    if (scheme == 0) return launch_with_lds(sojourn_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, rows, row_ms, delay_bins, delay_bin_ms, rcap, out);
    return launch_with_lds(sojourn_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, rows, row_ms, delay_bins, delay_bin_ms, rcap, out);
}

} // namespace prach
