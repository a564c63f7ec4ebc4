// prach_noma_resolve.h — the NOMA grouping of ONE sector by ONE wavefront (NOMA.c:214-309 per sector / :341-437 cell-wide), device only.
// Written for both draw sources; included by prach_noma.hip (Philox: one wavefront per sector, every workgroup of a cluster computes the same
// grouping).  prach_noma_glibc.hip (the reference's own rand() stream) keeps its own statement of the same algorithm, because its kernel gains SGPR
// spills through this one (the numbers: the comment there, and LABNOTES).  The count <= nGrantUL shortcut and the loop over the sectors stay with the
// callers.  Double arithmetic here must not be contracted: the includers carry `#pragma clang fp contract(off)` (and the build -ffp-contract=off).
#pragma once
#include "prach_device_fn.h"
#include "prach_noma_act.h"

namespace prach {

struct NomaGain { double gain, lgain; };           // channelGain and its natural log
struct NomaResolved { bool ambiguous; int status; }; // (both wave-uniform)

__device__ __forceinline__ void noma_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane = preamble.  single / myidx: this lane's preamble has exactly one transmitter in the sector, and which; more than nGrantUL of them (the
// caller's shortcut took the other case).  Singleton transmitters in preamble order (ballot compaction into the LDS staging arrays sidx / sg / slg,
// 64 entries each), stable ascending rank by gain == the reference's bubble sort with strict < (NOMA.c:90-103), greedy pairing over the sorted
// lanes (ballot + find-first), leftovers while grants remain.
//   gain_of(idx) -> NomaGain                 the UE's activation-table entry
//   draw(grant, which, d) -> bool            decode draw `which` (0, 1) of the sector's grant-th pair into d; false: none left (PRACH_ERR_STREAM:
//                                            the pairing stops and no grant of this sector is applied)
//   grant(idx)                               called by the lane that holds a granted UE
//   stamp(k)                                 diagnostic build: phase stamps 8 (gains loaded), 9 (ranked and sorted), 10 (paired); else empty
// devact != 0: the gains come from the device's libm — every comparison of gains is checked against its error band and reported (`ambiguous`:
// the caller has the trial rerun with the host-built table); devact == 2: test hook, every sort counts as ambiguous.
template <class GAIN, class DRAW, class GRANT, class STAMP>
__device__ __forceinline__ NomaResolved noma_resolve_sector(const bool single, const int myidx, const int nGrantUL, const bool nonsector, const int devact,
                                                            int *const sidx, double *const sg, double *const slg, GAIN &&gain_of, DRAW &&draw, GRANT &&grant, STAMP &&stamp) {
    const int lane = threadIdx.x & 63;
    const unsigned long long sm = __ballot(single);
    const int count = __popcll(sm);
    int status = PRACH_OK;
    if (single) { const int q = __popcll(sm & lanemask_lt(lane)); const NomaGain g = gain_of(myidx); sidx[q] = myidx; sg[q] = g.gain; slg[q] = g.lgain; }
    noma_wave_sync();
    stamp(8);
    int uidx = -1, rank = 0;
    double ug = 0, ulg = 0;
    bool ambiguous = false;
    if (lane < count) {
        uidx = sidx[lane]; ug = sg[lane]; ulg = slg[lane];
#pragma unroll 8
        for (int j = 0; j < count; j++) { // (unrolled: eight broadcast reads in flight instead of one LDS round trip per comparison)
            const double gj = sg[j];
            rank += (gj < ug || (gj == ug && j < lane)) ? 1 : 0;
        }
    }
    noma_wave_sync();
    if (lane < count) { sidx[rank] = uidx; slg[rank] = ulg; sg[rank] = ug; } // (every lane has read the unsorted gains: barrier above)
    noma_wave_sync();
    int cidx = -1;
    double clg = 0;
    if (lane < count) { cidx = sidx[lane]; clg = slg[lane]; }
    // device-built table: two gains closer than the error band of the device's libm (ACT_GAIN_ORDER_BAND, prach_noma_act.h: twice the asserted
    // per-gain error, with margin) could be ordered the other way by the reference's — in sorted order it is enough to look at neighbours
    if (devact && lane + 1 < count) { const double ga = sg[lane], gb = sg[lane + 1]; if (__dsub_rn(gb, ga) <= ACT_GAIN_ORDER_BAND * gb || devact == 2) ambiguous = true; }
    stamp(9);
    unsigned long long valid = count >= 64 ? ~0ull : ((1ull << count) - 1ull);
    const double clg10 = __dmul_rn(10.0, clg); // (NOMA.c:272: 10 * log(gain), the same product on either side of the difference)
    int grants = 0;
    bool grantme = false;
    const unsigned long long lows = count >= 2 ? ((1ull << (count - 1)) - 1ull) : 0ull; // i < count - 1
    unsigned long long above = ~0ull;                                                    // bits behind the last i looked at
    for (;;) { // NOMA.c:268-298 (enNoma stays 0: :266,269), over the still unpaired i in ascending order
        const unsigned long long rest = valid & lows & above;
        if (!rest) break;
        const int i = __ffsll((long long)rest) - 1;
        above = ~((2ull << i) - 1ull);
        // (lane i's 10 ln g through two v_readlane — i is wave-uniform — instead of a ds_bpermute round trip per comparison: this loop is a latency chain)
        const double lgi10 = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(clg10), i), __builtin_amdgcn_readlane(__double2loint(clg10), i));
        const double diff = __dsub_rn(clg10, lgi10); // 10*log(high) - 10*log(low)
        if (devact && lane < count && fabs(__dsub_rn(diff, 15.0)) < 1e-9) ambiguous = true; // (|error| of 10 ln g1 - 10 ln g2 < 1e-12; at worst one more rerun with the host's table)
        // (the lanes still unpaired, not lane 0, not i itself: scalar mask algebra on the comparison's ballot instead of a 64-bit shift per lane)
        const unsigned long long mj = __ballot(diff > 15.0) & valid & ~(1ull << i) & ~1ull;
        if (!mj) continue;
        const int j = __ffsll((long long)mj) - 1;
        valid &= ~((1ull << i) | (1ull << j));
        if (grants < nGrantUL) {
            const int g = grants++;
            int d1, d2, decoded = 2; // both
            if (!draw(g, 0, d1)) { status = PRACH_ERR_STREAM; break; }
            // (double)rand() / RAND_MAX < 0.3 (NOMA.c:284-285), on the integer: for a 31-bit d, (double)d / 2147483647.0 < 0.3 exactly when d <= 644245094
            // (644245094 gives 0.29999999995, 644245095 gives 0.3000000004: both five orders of magnitude further from 0.3 than a double's rounding)
            if (d1 <= 644245094) {
                if (nonsector) decoded = 0; // rx[0], the weaker UE: NOMA.c:413-415
                else {
                    if (!draw(g, 1, d2)) { status = PRACH_ERR_STREAM; break; }
                    decoded = d2 % 2; // NOMA.c:287-290: index into rx[] = {low, high}
                }
            }
            if ((lane == i && (decoded == 2 || decoded == 0)) || (lane == j && (decoded == 2 || decoded == 1))) grantme = true;
        }
    }
    { // leftovers in sorted order while grants remain (NOMA.c:299-307)
        const bool left = lane < count && ((valid >> lane) & 1ull);
        const unsigned long long lm = __ballot(left);
        if (left && __popcll(lm & lanemask_lt(lane)) < nGrantUL - grants) grantme = true;
    }
    stamp(10);
    if (grantme && status == PRACH_OK) grant(cidx);
    return NomaResolved{__any(ambiguous) != 0, status};
}

} // namespace prach
