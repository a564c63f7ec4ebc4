// prach_resolve.h — the resolver's two steps in front of the scan counts, ONE copy (device only): every gathered event against the first-caller
// table, and the reset-cycle candidates in index order.  Included by prach_cluster.hip, prach_lcluster.hip and prach_batch.hip; what differs between
// them — where event k lives and where the tables are — comes in as accessors and pointers.  (trial_kernel's sequential resolver, prach_kernels.hip,
// is a different algorithm.)
#pragma once
#include "prach_device_fn.h"
#include "prach_ue_body.h"
#include <limits.h>

namespace prach {

// Event info word (20 bits): type[2:0] ispre[3] bucket p[11:4] old bucket q[19:12].  Types: the per-UE body's UEV_* (prach_ue_body.h) and
constexpr int EV_LEAVER = 4; // an early leaver below its bucket's lowest caller (appended by the workgroup, not by the per-UE body)

struct ResolveTables {
    int *fcall, *nlv, *fie; // per bucket: lowest definite caller, leavers below it, "the first caller is an event"
    int *rclist, *sidx;     // [RCCAP] event numbers of the surviving reset-cycle candidates; the same, sorted (any free space)
    int *nrc, *nrj;         // counters: candidates listed, re-joins
};

// One gathered event (number k, value ev) against the lowest DEFINITE caller of every bucket (complete after round 1).  kill(k): event k is void.
template <class KILL>
__device__ __forceinline__ void classify_event(const ResolveTables &R, const int k, const int2 ev, KILL &&kill) {
    const int type = ev.y & 7, p = (ev.y >> 4) & 0xff;
    if (type == UEV_RESETCAND) {
        // a call on its old bucket by a definite caller with a lower index bumps it: cannot re-join (99.7 % of
        // them); only the survivors need the index-ordered treatment
        if (R.fcall[(ev.y >> 12) & 0xff] < ev.x) kill(k);
        else { const int s = atomicAdd(R.nrc, 1); if (s < RCCAP) R.rclist[s] = k; }
    } else if (type == UEV_RJOIN) {
        atomicAdd(R.nrj, 1);
    } else if (type == EV_LEAVER) {
        if (ev.x < R.fcall[p]) atomicAdd(&R.nlv[p], 1);
    } else if (type == UEV_CALLER) {
        if (ev.x == R.fcall[p]) R.fie[p] = 1;
    }
}

// Reset-cycle candidates (Beta.c:250-281 with tmp == 0 on a subframe = 1 mod accessTime): candidate i
// re-joins (and calls on its NEW preamble) iff nobody called on its OLD preamble before it, and a
// re-join is itself a call that later candidates must see.  Inherently sequential in index order,
// but tiny: ONE wavefront keeps the per-bucket first-caller table in registers (lane = bucket, NB = 1 or 4
// registers of 64 buckets) and walks the index-sorted candidates with v_readlane — no LDS round trip per step.
// get(k) -> int2: event k; kill(k): event k is void.
template <int NB>
__device__ __forceinline__ int fc_get(const int f0, const int f1, const int f2, const int f3, const int q) {
    const int l = q & 63;
    if constexpr (NB == 1) return __builtin_amdgcn_readlane(f0, l);
    else switch (q >> 6) {
        case 0: return __builtin_amdgcn_readlane(f0, l);
        case 1: return __builtin_amdgcn_readlane(f1, l);
        case 2: return __builtin_amdgcn_readlane(f2, l);
        default: return __builtin_amdgcn_readlane(f3, l);
    }
}
template <int NB, class GET, class KILL>
__device__ __forceinline__ void resolve_reset_candidates(const ResolveTables &R, const int nrc_in, const int nP, GET &&get, KILL &&kill) {
    static_assert(NB == 1 || NB == 4, "one or four registers of 64 buckets");
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(nrc_in);
    int f0 = lane < nP ? R.fcall[lane] : INT_MAX, f1 = INT_MAX, f2 = INT_MAX, f3 = INT_MAX; // (NB == 1: f1 .. f3 are never looked at)
    if constexpr (NB == 4) {
        f1 = lane + 64 < nP ? R.fcall[lane + 64] : INT_MAX; f2 = lane + 128 < nP ? R.fcall[lane + 128] : INT_MAX; f3 = lane + 192 < nP ? R.fcall[lane + 192] : INT_MAX;
    }
    for (int c = lane; c < n; c += 64) { // rank-sort the candidate list by UE index into sidx (free at this point of the subframe)
        const int myidx = get(R.rclist[c]).x;
        int rank = 0;
        for (int j = 0; j < n; j++) rank += get(R.rclist[j]).x < myidx ? 1 : 0;
        R.sidx[rank] = R.rclist[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int base = 0; base < n; base += 64) {
        const int m = min(64, n - base);
        int es = 0, cidx = 0, cinfo = 0;
        if (lane < m) { es = R.sidx[base + lane]; const int2 e = get(es); cidx = e.x; cinfo = e.y; }
        int cancelled = 0;
        for (int s_ = 0; s_ < m; s_++) {
            const int idx = __builtin_amdgcn_readlane(cidx, s_), info = __builtin_amdgcn_readlane(cinfo, s_);
            const int p = (info >> 4) & 0xff, q = (info >> 12) & 0xff;
            if (fc_get<NB>(f0, f1, f2, f3, q) < idx) { // bumped before its turn: does not re-join
                if (lane == s_) cancelled = 1;
            } else if (idx < fc_get<NB>(f0, f1, f2, f3, p)) { // its call becomes the first one on p
                if (lane == (p & 63)) {
                    if constexpr (NB == 1) f0 = idx;
                    else switch (p >> 6) { case 0: f0 = idx; break; case 1: f1 = idx; break; case 2: f2 = idx; break; default: f3 = idx; break; }
                }
            }
        }
        if (lane < m && cancelled) kill(es);
    }
    if (lane < nP) R.fcall[lane] = f0;
    if constexpr (NB == 4) {
        if (lane + 64 < nP) R.fcall[lane + 64] = f1;
        if (lane + 128 < nP) R.fcall[lane + 128] = f2;
        if (lane + 192 < nP) R.fcall[lane + 192] = f3;
    }
}

} // namespace prach
