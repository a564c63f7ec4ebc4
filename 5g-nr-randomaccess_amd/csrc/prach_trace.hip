// prach_trace.hip — prach::trace_kernel: per trial group, the preambles used, decoded and collided in each stretch of the simulation (include/prach.h,
// prach_run_trials_trace), reduced on the device from the per-subframe rows the simulation kernels write while they run (TrialDev::trace: calls, singles,
// txop, collisions of every subframe; a subframe without a call keeps the zeros the engine put there).  gfx950 only.  The definition is the plain loop over
// the rows (tests/tools/gpu_trace_harness.hip has it as its host reference): every row adds to the scalars, and to bin t / bin_ms of the four series unless
// that bin lies at or behind `bins` — then its calls count in overflow_calls and in no bin.
//
// The engine launches it on its stream behind a simulation launch, for the trials whose result it keeps.  A workgroup takes ONE tile of TR_TILE consecutive
// subframes of ONE trial (the job table gives every trial its first workgroup); lane l of a pass loads row first + pass * TR_THREADS + l with one 16-byte
// load, so a wavefront reads 1 KiB in one piece.  Consecutive subframes share a bin, and a tile covers at most TR_TILE consecutive bins from bin first / bin_ms
// on.  SCHEME 1 adds the rows up in an LDS window of four 64-bit counters per bin anchored there, and flushes the non-zero counters with 64-bit agent-scope
// atomic adds (trials of one group run on different XCDs).  SCHEME 0 sends every non-zero contribution straight to the global bins with the same atomics.
// The scalars are reduced per wavefront.  Integers only: the result does not depend on any order.  Engine option "trace_scheme"; DESIGN.md 4 has the
// measurements.  A row's words are counts, read as unsigned 32-bit values and added in 64 bits.
#include "prach_reduce_tile.h"

namespace prach {

namespace {

template <int SCHEME>
__global__ __launch_bounds__(TR_THREADS) void trace_kernel(const TraceJob *__restrict__ jobs, int njobs, int bins, int width, TraceOut out) {
    extern __shared__ unsigned long long lds64[]; // [TR_SCALARS] scalars | SCHEME 1: [TR_TILE][4] the window
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long *const lsc = lds64;
    unsigned long long *const lwin = lds64 + TR_SCALARS;

    const TraceJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TR_TILE;
    const int end = min(J.steps, first + TR_TILE);
    if (first >= end) return; // (uniform: a job without subframes has no tile)
    const unsigned bin0 = (unsigned)first / (unsigned)width;
    const int nwin = min((int)((unsigned)(end - 1) / (unsigned)width - bin0) + 1, TR_TILE); // bins this tile touches (at most one per subframe)
    if (SCHEME == 1)
        for (int b = tid; b < 4 * nwin; b += TR_THREADS) lwin[b] = 0;
    if (tid < TR_SCALARS) lsc[tid] = 0;
    __syncthreads();

    const size_t gbase = (size_t)J.group * (size_t)bins;
    unsigned long long calls = 0, singles = 0, txop = 0, coll = 0, over = 0;
    unsigned cmax1 = 0;
    for (int t = first + tid; t < end; t += TR_THREADS) {
        const int4 r = J.rows[t];
        const unsigned c = (unsigned)r.x, s = (unsigned)r.y, x = (unsigned)r.z, q = (unsigned)r.w;
        cmax1 = max(cmax1, min(c, 0xFFFFFFFEu) + 1u);
        calls += c; singles += s; txop += x; coll += q;
        const unsigned b = width == 1 ? (unsigned)t : (unsigned)t / (unsigned)width;
        if (b >= (unsigned)bins) { over += c; continue; }
        if (SCHEME == 1) {
            unsigned long long *const w = lwin + 4 * (size_t)(b - bin0);
            if (c) atomicAdd(&w[0], (unsigned long long)c);
            if (s) atomicAdd(&w[1], (unsigned long long)s);
            if (x) atomicAdd(&w[2], (unsigned long long)x);
            if (q) atomicAdd(&w[3], (unsigned long long)q);
        } else {
            if (c) agent_add(&out.calls[gbase + b], (unsigned long long)c);
            if (s) agent_add(&out.singles[gbase + b], (unsigned long long)s);
            if (x) agent_add(&out.txop[gbase + b], (unsigned long long)x);
            if (q) agent_add(&out.collisions[gbase + b], (unsigned long long)q);
        }
    }
    calls = fold_sum(calls); singles = fold_sum(singles); txop = fold_sum(txop); coll = fold_sum(coll); over = fold_sum(over); cmax1 = fold_max(cmax1);
    if (lane == 0) {
        atomicAdd(&lsc[1], calls); atomicAdd(&lsc[2], singles); atomicAdd(&lsc[3], txop); atomicAdd(&lsc[4], coll); atomicAdd(&lsc[5], over);
        atomicMax(&lsc[6], (unsigned long long)cmax1);
    }
    if (tid == 0) lsc[0] = (unsigned long long)(end - first); // (zeroed in front of the barrier above; nobody else writes it)
    __syncthreads();

    // flush: only what this tile touched (a window bin that was added to lies below `bins`)
    if (SCHEME == 1) {
        for (int b = tid; b < nwin; b += TR_THREADS) {
            const unsigned long long *const w = lwin + 4 * (size_t)b;
            const size_t at = gbase + (size_t)bin0 + (size_t)b;
            const unsigned long long v0 = w[0], v1 = w[1], v2 = w[2], v3 = w[3];
            if (v0) agent_add(&out.calls[at], v0);
            if (v1) agent_add(&out.singles[at], v1);
            if (v2) agent_add(&out.txop[at], v2);
            if (v3) agent_add(&out.collisions[at], v3);
        }
    }
    flush_scalars(lsc, out.scalars + (size_t)J.group * TR_SCALARS, TR_SUMS, TR_MAXIMA, tid);
}

size_t trace_lds_bytes(int scheme) { return 8 * (size_t)(TR_SCALARS + (scheme == 1 ? 4 * TR_TILE : 0)); }

} // namespace

hipError_t launch_trace_kernel(const TraceJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, TraceOut out, hipStream_t stream) {
    const size_t lds = trace_lds_bytes(scheme);
    if (scheme == 0) return launch_with_lds(trace_kernel<0>, workgroups, TR_THREADS, lds, stream, jobs, njobs, bins, bin_ms, out);
    return launch_with_lds(trace_kernel<1>, workgroups, TR_THREADS, lds, stream, jobs, njobs, bins, bin_ms, out);
}

} // namespace prach
