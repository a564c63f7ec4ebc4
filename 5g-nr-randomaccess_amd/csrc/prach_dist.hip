// prach_dist.hip — prach::dist_kernel: the distributions of access delay and of the number of preamble transmissions of the successful UEs
// (include/prach.h, prach_run_trials_dist), reduced on the device from what a simulation kernel leaves there: timers[i] (the delay of a successful UE,
// INT_MIN otherwise) and preambleTxCounter (an int32 array, or word 5 of prach::batch_kernel's 32-byte records).  gfx950 only.
//
// The engine launches it on its stream behind a simulation launch, for the trials whose result it keeps.  A workgroup takes ONE tile of DIST_TILE UEs of
// ONE trial (the job table gives every trial its first workgroup): it zeroes delay_bins + 256 32-bit bins in LDS, reads its tile 16 bytes per lane, bins
// with non-returning LDS adds, reduces the scalars per wavefront and flushes only its non-zero bins with 64-bit device-scope atomic adds (trials of one
// group run on different XCDs) into the buffers the engine owns for the whole call.  Integers only: the result does not depend on any order.
//
// SCHEME: how the preamble counts are binned (the delays are spread over tens of bins and more; the counts of an overloaded trial sit in a handful,
// and same-address LDS atomics serialise): 0 one LDS add per UE; 1 the same into a copy of the 256 bins per wavefront; 2 one LDS add per distinct
// value of a wavefront (match and aggregate).  Engine option "dist_scheme"; DESIGN.md 4 has the measurements.
#include "prach_reduce_tile.h"

#include <limits.h>

namespace prach {

namespace {

constexpr int DIST_WAVES = DIST_THREADS / 64;
constexpr int PB = PRACH_DIST_PTC_BINS;

template <int SCHEME>
__global__ __launch_bounds__(DIST_THREADS) void dist_kernel(const DistJob *__restrict__ jobs, int njobs, int bins, int width, unsigned long long *__restrict__ dh,
                                                            unsigned long long *__restrict__ ph, unsigned long long *__restrict__ sc) {
    extern __shared__ unsigned lds[]; // [bins] delay | [PB x copies] preamble counts | 5 x 64-bit scalars
    constexpr int COPIES = SCHEME == 1 ? DIST_WAVES : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned *const ldel = lds;
    unsigned *const lptc = lds + bins;
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + ((bins + PB * COPIES + 1) & ~1));

    const DistJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * DIST_TILE;
    const int end = min(J.nUE, first + DIST_TILE);

    for (int b = tid; b < bins + PB * COPIES; b += DIST_THREADS) lds[b] = 0;
    if (tid < DIST_SUMS + DIST_MAXIMA) lsc[tid] = 0;
    __syncthreads();

    unsigned nsucc = 0, nover = 0, dmax1 = 0;
    unsigned long long dsum = 0, psum = 0;
    unsigned *const myptc = lptc + (SCHEME == 1 ? wave * PB : 0);
    const int *const rec5 = J.ptc + 5; // form 1: word 5 of UE i's 32-byte record is rec5[8 i]
    for (int base = first + 4 * tid; base < first + DIST_TILE; base += 4 * DIST_THREADS) { // (the same trip count in every lane: SCHEME 2 votes)
        int t[4], p[4];
        if (base + 4 <= end) {
            const int4 tv = *reinterpret_cast<const int4 *>(J.timers + base); // (arena offsets are 256-byte aligned, base is a multiple of 4)
            t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
            if (J.form == 0) {
                const int4 pv = *reinterpret_cast<const int4 *>(J.ptc + base);
                p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                t[c] = base + c < end ? J.timers[base + c] : INT_MIN;
                p[c] = (J.form == 0 && base + c < end) ? J.ptc[base + c] : 0;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const bool ok = t[c] != INT_MIN;
            if (J.form != 0) p[c] = ok ? (rec5[8 * (size_t)(base + c)] & 0xffff) : 0; // (only the 32-byte sectors of successful UEs are read)
            const int pbin = (int)min((unsigned)p[c], (unsigned)(PB - 1));
            if (ok) {
                const unsigned d = (unsigned)t[c];
                const unsigned b = width == 1 ? d : d / (unsigned)width;
                if (b < (unsigned)bins) atomicAdd(&ldel[b], 1u); else nover++;
                nsucc++;
                dsum += d;
                psum += (unsigned)p[c];
                dmax1 = max(dmax1, d + 1u);
                if (SCHEME != 2) atomicAdd(&myptc[pbin], 1u);
            }
            if (SCHEME == 2) { // every lane of the wavefront is here: one add per distinct value
                unsigned long long todo = __ballot(ok);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int v = __shfl(pbin, leader);
                    const unsigned long long same = __ballot(ok && pbin == v);
                    if (lane == leader) atomicAdd(&myptc[v], (unsigned)__popcll(same));
                    todo &= ~same;
                }
            }
        }
    }
    nsucc = fold_sum(nsucc); nover = fold_sum(nover); dsum = fold_sum(dsum); psum = fold_sum(psum); dmax1 = fold_max(dmax1);
    if (lane == 0 && nsucc) {
        atomicAdd(&lsc[0], (unsigned long long)nsucc); atomicAdd(&lsc[1], (unsigned long long)nover); atomicAdd(&lsc[2], dsum); atomicAdd(&lsc[3], psum);
        atomicMax(&lsc[4], (unsigned long long)dmax1);
    }
    __syncthreads();

    // flush: only what this tile touched
    unsigned long long *const gdh = dh + (size_t)J.group * (size_t)bins;
    unsigned long long *const gph = ph + (size_t)J.group * PB;
    for (int b = tid; b < bins; b += DIST_THREADS) {
        const unsigned v = ldel[b];
        if (v) agent_add(&gdh[b], (unsigned long long)v);
    }
    for (int b = tid; b < PB; b += DIST_THREADS) {
        unsigned v = 0;
#pragma unroll
        for (int q = 0; q < COPIES; q++) v += lptc[q * PB + b];
        if (v) agent_add(&gph[b], (unsigned long long)v);
    }
    flush_scalars(lsc, sc + (size_t)J.group * DIST_SCALARS, DIST_SUMS, DIST_MAXIMA, tid);
}

size_t dist_lds_bytes(int bins, int scheme) {
    const int copies = scheme == 1 ? DIST_WAVES : 1;
    return 4 * (size_t)((bins + PB * copies + 1) & ~1) + 8 * 5;
}

} // namespace

hipError_t launch_dist_kernel(const DistJob *jobs, int njobs, int workgroups, int delay_bins, int delay_bin_ms, int scheme, unsigned long long *delay_hist,
                              unsigned long long *ptc_hist, unsigned long long *scalars, hipStream_t stream) {
    const size_t lds = dist_lds_bytes(delay_bins, scheme);
    switch (scheme) {
    case 0: return launch_with_lds(dist_kernel<0>, workgroups, DIST_THREADS, lds, stream, jobs, njobs, delay_bins, delay_bin_ms, delay_hist, ptc_hist, scalars);
    case 1: return launch_with_lds(dist_kernel<1>, workgroups, DIST_THREADS, lds, stream, jobs, njobs, delay_bins, delay_bin_ms, delay_hist, ptc_hist, scalars);
    default: return launch_with_lds(dist_kernel<2>, workgroups, DIST_THREADS, lds, stream, jobs, njobs, delay_bins, delay_bin_ms, delay_hist, ptc_hist, scalars);
    }
}

} // namespace prach
