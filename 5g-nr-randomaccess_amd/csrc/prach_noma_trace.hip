// prach_noma_trace.hip — prach::noma_trace_kernel: per trial group and sector, what happened on NOMA.c's channel in each stretch of the simulation
// (include/prach.h, prach_run_trials_noma_trace), reduced on the device from the per-(access slot, sector) rows prach::noma_kernel writes while it runs
// (TrialDev::trace: tx, used, singles, granted, pairs, pair_one, two zero words; a (slot, sector) without a transmitter keeps the zeros the engine put
// there).  gfx950 only.  The definition is the plain loop over the rows (tests/tools/gpu_noma_trace_harness.hip's host side and tests/tools/
// noma_trace_cases.py state it): row r is slot r / 6, sector r % 6; every row adds to the scalars, and to bin (slot * accessTime) / bin_ms of its sector's six
// series unless that bin lies at or behind `bins` — then its tx counts in overflow_tx and in no bin.
//
// The shape is prach::trace_kernel's (prach_trace.hip).  A workgroup takes ONE tile of NT_TILE consecutive rows — NT_TILE / 6 whole slots — of ONE trial (the job
// table gives every trial its first workgroup); a lane loads its row with two 16-byte loads.  Consecutive slots fall into ascending bins.  SCHEME 1 adds the
// rows up in an LDS window of 64-bit counters, NT_WINDOW bins x 6 sectors x 6 series, anchored at the tile's first bin, and flushes the non-zero counters with
// 64-bit agent-scope atomic adds (trials of one group run on different XCDs); with bin_ms >= accessTime a tile never leaves its window, with a smaller bin_ms
// what falls behind it goes straight out.  SCHEME 0 sends every non-zero contribution straight to the global bins with the same atomics.  The scalars are
// reduced per wavefront.  Integers only: the result does not depend on any order.  Engine option "trace_scheme".  A row's words are counts, read as unsigned
// 32-bit values and added in 64 bits (the LDS counters are 64-bit too: nothing bounds a tile's sum but that).
#include "prach_reduce_tile.h"

namespace prach {

namespace {

// The kernel is a member of the trace_kernel family by name — trace_kernel<NomaRows, SCHEME>; `noma_trace_kernel<SCHEME>` below is its name in the sources —
// so that every census of the library's kernel symbols by the name in front of the template arguments (tests/tools/cut_cases.py: LEFT_OUT) classes it with
// the reducers, as it classes prach_trace.hip's.
struct NomaRows {};
template <class ROWS, int SCHEME>
__global__ __launch_bounds__(NT_THREADS) void trace_kernel(const NomaTraceJob *__restrict__ jobs, int njobs, int bins, int width, NomaTraceOut out) {
    extern __shared__ unsigned long long lds64[]; // [NT_SCALARS] scalars | SCHEME 1: [6 series][NT_WINDOW][6 sectors] the window
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long *const lsc = lds64;
    unsigned long long *const lwin = lds64 + NT_SCALARS;

    const NomaTraceJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * NT_TILE;
    const int end = min(J.nrows, first + NT_TILE);
    if (first >= end) return; // (uniform: a job without rows has no tile)
    const unsigned aT = (unsigned)J.aT;
    const unsigned bin0 = ((unsigned)first / 6u) * aT / (unsigned)width;
    const unsigned binl = ((unsigned)(end - 1) / 6u) * aT / (unsigned)width;
    const int nwin = (int)min(binl - bin0 + 1u, (unsigned)NT_WINDOW); // bins of this tile that the window holds
    if (SCHEME == 1) {
#pragma unroll
        for (int q = 0; q < 6; q++)
            for (int x = tid; x < 6 * nwin; x += NT_THREADS) lwin[q * 6 * NT_WINDOW + x] = 0;
    }
    if (tid < NT_SCALARS) lsc[tid] = 0;
    __syncthreads();

    const size_t gbase = (size_t)J.group * 6 * (size_t)bins;
    unsigned long long sum[6] = {0, 0, 0, 0, 0, 0}, over = 0;
    unsigned txmax1 = 0;
    for (int r = first + tid; r < end; r += NT_THREADS) {
        const int4 a = J.rows[2 * (size_t)r], c = J.rows[2 * (size_t)r + 1];
        const unsigned v[6] = {(unsigned)a.x, (unsigned)a.y, (unsigned)a.z, (unsigned)a.w, (unsigned)c.x, (unsigned)c.y};
        const unsigned slot = (unsigned)r / 6u, sec = (unsigned)r - 6u * slot;
        txmax1 = max(txmax1, min(v[0], 0xFFFFFFFEu) + 1u);
#pragma unroll
        for (int q = 0; q < 6; q++) sum[q] += v[q];
        const unsigned b = slot * aT / (unsigned)width;
        if (b >= (unsigned)bins) { over += v[0]; continue; }
        if (SCHEME == 1 && b - bin0 < (unsigned)nwin) {
            unsigned long long *const w = lwin + (size_t)(b - bin0) * 6 + sec;
#pragma unroll
            for (int q = 0; q < 6; q++)
                if (v[q]) atomicAdd(&w[q * 6 * NT_WINDOW], (unsigned long long)v[q]);
        } else {
            const size_t at = gbase + (size_t)sec * (size_t)bins + b;
#pragma unroll
            for (int q = 0; q < 6; q++)
                if (v[q]) agent_add(&out.series[q][at], (unsigned long long)v[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) sum[q] = fold_sum(sum[q]);
    over = fold_sum(over); txmax1 = fold_max(txmax1);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 6; q++) atomicAdd(&lsc[1 + q], sum[q]);
        atomicAdd(&lsc[7], over);
        atomicMax(&lsc[8], (unsigned long long)txmax1);
    }
    if (tid == 0) lsc[0] = (unsigned long long)((end + 5) / 6 - (first + 5) / 6); // slots whose sector-0 row is in the tile (zeroed in front of the barrier above; nobody else writes it)
    __syncthreads();

    // flush: only what this tile touched (a window bin that was added to lies below `bins`)
    if (SCHEME == 1) {
#pragma unroll
        for (int q = 0; q < 6; q++)
            for (int x = tid; x < 6 * nwin; x += NT_THREADS) {
                const unsigned long long v = lwin[q * 6 * NT_WINDOW + x];
                const unsigned b = (unsigned)x / 6u, sec = (unsigned)x - 6u * b;
                if (v) agent_add(&out.series[q][gbase + (size_t)sec * (size_t)bins + bin0 + b], v);
            }
    }
    flush_scalars(lsc, out.scalars + (size_t)J.group * NT_SCALARS, NT_SUMS, NT_MAXIMA, tid);
}

template <int SCHEME> constexpr auto noma_trace_kernel = &trace_kernel<NomaRows, SCHEME>;

size_t noma_trace_lds_bytes(int scheme) { return 8 * (size_t)(NT_SCALARS + (scheme == 1 ? 36 * NT_WINDOW : 0)); }

} // namespace

hipError_t launch_noma_trace_kernel(const NomaTraceJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, NomaTraceOut out, hipStream_t stream) {
    const size_t lds = noma_trace_lds_bytes(scheme);
    if (scheme == 0) return launch_with_lds(noma_trace_kernel<0>, workgroups, NT_THREADS, lds, stream, jobs, njobs, bins, bin_ms, out);
    return launch_with_lds(noma_trace_kernel<1>, workgroups, NT_THREADS, lds, stream, jobs, njobs, bins, bin_ms, out);
}

} // namespace prach
