// prach_noma_gain.hip — NOMA.c's near-far profile (include/prach.h, prach_run_trials_noma_gain): per trial group, SECTOR and channel-gain LEVEL, what became of
// the UEs of a NOMA.c trial, reduced on the device from the 64-byte per-UE log records prach::noma_kernel writes there, the trial's arrival schedule, its `steps`
// and the ln(gain) column of the launch's activation table.  gfx950 only.  prach_noma_gain_accumulate_levels (prach_host.c) is the definition; the reducer
// equals it integer for integer.  Two kernels:
//
// THE LEVEL PRE-PASS, noma_gain_levels_kernel: one thread per UE writes L = floor(1000 x lgain) into the job's 4-byte level column — the product is
// __dmul_rn, the host's one IEEE multiplication.  Where the table was built on the device (n_devact) lgain may differ from the host libm's in the last bits, so a
// UE whose product lies within NG_LEVEL_BAND of an integer (prach_device.h derives the band), outside the range the band is derived for, or that has no level
// is EDGE: it is appended to a bounded list, and the engine resolves exactly those UEs with the host's libm before the reducer starts.  The count goes on
// counting past the capacity (the engine then builds every level of the launch on the host); no entry is written past it.
//
// THE REDUCER, noma_gain_kernel: the reducers' shape — a workgroup takes ONE tile of TL_TILE consecutive UEs of ONE trial (prach_reduce_tile.h: job lookup,
// slot range of the tile, folds, flush of the scalars); the job's `pad` carries E = min(steps, maxTime).  Class and values are THE NOMA MENU's
// (prach_noma_menu.h), not a second statement of it: quarters 0 (timer, txTime), 2 (the sector, the preamble count) and 3 (msg4Flag, failCount), never quarter 1.
// A tile's UEs scatter over the whole gain axis, so there is no anchored window: SCHEME 1 holds ALL 6 series x 6 sectors x bins 32-bit counters of the tile in
// LDS (the launch picks it only for bins <= NG_LDS_MAX_BINS: two workgroups per CU) and flushes the non-zero ones with 64-bit agent-scope atomic adds; an
// addend above NG_MAX_ADDEND (no trial produces one; the definition takes any value >= 0) goes straight out.  SCHEME 0 sends everything straight out.  The
// scalars are reduced per wavefront.  Integers only: the result does not depend on any order.  Engine option "timeline_scheme"; profiles/noma_gain_kernel.md.
#include "prach_reduce_tile.h"
#include "prach_noma_menu.h"
#include "prach_noma_act.h"

namespace prach {

static_assert(ACT_GAIN_ULP_ASSERTED == 32, "NG_LEVEL_ERROR (prach_device.h) is derived from this bound on the gains of a device-built table");
static_assert((unsigned long long)TL_TILE * NG_MAX_ADDEND < (1ull << 32), "a 32-bit LDS counter holds each of the three sums of a whole tile");

namespace {

// Both kernels are members of families the library already has, by name — noma_columns_kernel<NomaGainLevels> writes a per-UE int32 column as
// prach_noma_census.hip's does, noma_census_kernel<NomaGainUes, SCHEME> is a census of NOMA.c's UEs over another axis (the timeline_kernel family is closed: its
// four members are listed by name elsewhere) — so that every census of the library's kernel symbols by the name in front of the template arguments
// (tests/tools/cut_cases.py: LEFT_OUT) classes them with the reducers.
struct NomaGainLevels {};
struct NomaGainUes {};

template <class WHAT>
__global__ __launch_bounds__(TL_THREADS) void noma_columns_kernel(const NomaGainJob *__restrict__ jobs, int njobs, unsigned *__restrict__ edges, int edge_cap) {
    int jlo = 0, jhi = njobs - 1; // job_of_workgroup's search, for the job's index: what an EDGE UE is listed under
    while (jlo < jhi) {
        const int mid = (jlo + jhi + 1) >> 1;
        if (jobs[mid].wg0 <= (int)blockIdx.x) jlo = mid; else jhi = mid - 1;
    }
    const NomaGainJob J = jobs[jlo];
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    for (int i = first + (int)threadIdx.x; i < end; i += TL_THREADS) {
        const double p = __dmul_rn(1000.0, J.lgain[i]);
        const bool has = fabs(p) < 1073741824.0; // (false for a NaN and for an infinity)
        const double f = floor(p);
        J.level[i] = has ? (int)f : INT32_MIN;
        const double d = p - f; // exact: 0 <= d < 1
        const bool edge = !has || !(fabs(p) < NG_LEVEL_RANGE) || d <= NG_LEVEL_BAND || d >= 1.0 - NG_LEVEL_BAND;
        if (edge) {
            const unsigned at = atomicAdd(&edges[0], 1u);
            if (at < (unsigned)edge_cap) {
                edges[2 + 2 * (size_t)at] = (unsigned)jlo;
                edges[3 + 2 * (size_t)at] = (unsigned)i;
            }
        }
    }
}

template <class UES, int SCHEME>
__global__ __launch_bounds__(TL_THREADS) void noma_census_kernel(const NomaGainJob *__restrict__ jobs, int njobs, int bins, int width, int lo, NomaGainOut out) {
    extern __shared__ unsigned lds[]; // [TILE_SCHED_CAP] schedule range | NG_SCALARS x 64-bit scalars | SCHEME 1: [6 series][6 sectors][bins] the tile's counters
    const int tid = threadIdx.x, lane = tid & 63;
    int *const lsched = reinterpret_cast<int *>(lds);
    unsigned long long *const lsc = reinterpret_cast<unsigned long long *>(lds + TILE_SCHED_CAP);
    unsigned *const lcnt = lds + TILE_SCHED_CAP + 2 * NG_SCALARS;

    const NomaGainJob J = job_of_workgroup(jobs, njobs);
    const int first = ((int)blockIdx.x - J.wg0) * TL_TILE;
    const int end = min(J.nUE, first + TL_TILE);
    const int E = J.pad;
    const unsigned nwords = 6u * (unsigned)bins; // words of one series of one group

    const TileSlots S = tile_slots<TL_THREADS>(J, first, end, lsched, tid);
    if (SCHEME == 1)
        for (unsigned x = tid; x < 6u * nwords; x += TL_THREADS) lcnt[x] = 0;
    if (tid < NG_SCALARS) lsc[tid] = 0;
    __syncthreads();

    const size_t gbase = (size_t)J.group * nwords;
    const NomaMenu::Needs needs{true, true, false}; // a(i), quarter 0, never quarter 1
    unsigned nidle = 0, nserved = 0, ndropped = 0, npending = 0, nundef = 0, nbelow = 0, nabove = 0, nrest = 0, ndef = 0, lmax1 = 0, nmax1 = 0;
    unsigned long long ssum = 0, lsum = 0, psum = 0;
    for (int i = first + tid; i < end; i += TL_THREADS) {
        const NomaMenu::Rec r = NomaMenu::load<false>(J.logs, i, needs);
        const int cls = NomaMenu::cls(r);
        const bool served = cls == PRACH_NOMA_SERVED, dropped = cls == PRACH_NOMA_DROPPED;
        nidle += cls == PRACH_NOMA_IDLE ? 1u : 0u;
        nserved += served ? 1u : 0u;
        ndropped += dropped ? 1u : 0u;
        npending += cls == PRACH_NOMA_PENDING ? 1u : 0u;
        if (cls == PRACH_NOMA_IDLE) continue;
        const int a = S.arrival(J, i);
        const int L = J.level[i];
        const long long sec = NomaMenu::value(PRACH_NOMA_SECTOR, r, cls, a, E);
        long long sj = 0, lost = 0, ptc = 0;
        if (served) {
            sj = NomaMenu::value(PRACH_NOMA_SOJOURN, r, cls, a, E);
            lost = NomaMenu::value(PRACH_NOMA_LOST, r, cls, a, E);
            ptc = NomaMenu::value(PRACH_NOMA_PTC, r, cls, a, E);
        }
        // undefined for the profile (the menu's ONE RULE: a negative value is undefined); min() over the values keeps this one compare
        if ((unsigned long long)sec > 5ull || L == INT32_MIN || min(min(sj, lost), ptc) < 0) { nundef++; continue; }
        ndef++;
        lmax1 = max(lmax1, (unsigned)L ^ 0x80000000u);       // L + 2^31 >= 1
        nmax1 = max(nmax1, (unsigned)(-L) ^ 0x80000000u);    // -L + 2^31 >= 1
        const bool below = L < lo;
        const unsigned b = ((unsigned)L - (unsigned)lo) / (unsigned)width; // where L >= lo: L - lo < 2^32, and b < bins iff L < lo + bins x width
        const bool in = !below && b < (unsigned)bins;
        nbelow += below ? 1u : 0u;
        nabove += !below && !in ? 1u : 0u;
        const unsigned wat = (unsigned)sec * (unsigned)bins + (in ? b : 0u); // in a series, where `in`
        if (in) {
            if (SCHEME == 1) atomicAdd(&lcnt[wat], 1u);
            else agent_add(&out.series[0][gbase + wat], 1ull);
            if (dropped) {
                if (SCHEME == 1) atomicAdd(&lcnt[2 * nwords + wat], 1u);
                else agent_add(&out.series[2][gbase + wat], 1ull);
            }
        }
        if (!served) continue;
        nrest += lost > 0 ? 1u : 0u;
        ssum += (unsigned long long)sj;
        lsum += (unsigned long long)lost;
        psum += (unsigned long long)ptc;
        if (!in) continue;
        if (SCHEME == 1 && max(max(sj, lost), ptc) <= NG_MAX_ADDEND) {
            atomicAdd(&lcnt[1 * nwords + wat], 1u);
            atomicAdd(&lcnt[3 * nwords + wat], (unsigned)sj);
            atomicAdd(&lcnt[4 * nwords + wat], (unsigned)lost);
            atomicAdd(&lcnt[5 * nwords + wat], (unsigned)ptc);
        } else {
            agent_add(&out.series[1][gbase + wat], 1ull);
            agent_add(&out.series[3][gbase + wat], (unsigned long long)sj);
            agent_add(&out.series[4][gbase + wat], (unsigned long long)lost);
            agent_add(&out.series[5][gbase + wat], (unsigned long long)ptc);
        }
    }
    nidle = fold_sum(nidle); nserved = fold_sum(nserved); ndropped = fold_sum(ndropped); npending = fold_sum(npending); nundef = fold_sum(nundef);
    nbelow = fold_sum(nbelow); nabove = fold_sum(nabove); nrest = fold_sum(nrest); ndef = fold_sum(ndef); ssum = fold_sum(ssum); lsum = fold_sum(lsum);
    psum = fold_sum(psum); lmax1 = fold_max(lmax1); nmax1 = fold_max(nmax1);
    if (lane == 0) {
        atomicAdd(&lsc[0], (unsigned long long)nidle); atomicAdd(&lsc[1], (unsigned long long)nserved); atomicAdd(&lsc[2], (unsigned long long)ndropped);
        atomicAdd(&lsc[3], (unsigned long long)npending); atomicAdd(&lsc[4], (unsigned long long)nundef); atomicAdd(&lsc[5], (unsigned long long)nbelow);
        atomicAdd(&lsc[6], (unsigned long long)nabove); atomicAdd(&lsc[7], (unsigned long long)nrest); atomicAdd(&lsc[8], ssum); atomicAdd(&lsc[9], lsum);
        atomicAdd(&lsc[10], psum); atomicAdd(&lsc[11], (unsigned long long)ndef);
        atomicMax(&lsc[12], (unsigned long long)lmax1); atomicMax(&lsc[13], (unsigned long long)nmax1);
    }
    __syncthreads();

    // flush: only what this tile touched
    if (SCHEME == 1) {
#pragma unroll
        for (int q = 0; q < 6; q++)
            for (unsigned x = tid; x < nwords; x += TL_THREADS) {
                const unsigned v = lcnt[q * nwords + x];
                if (v) agent_add(&out.series[q][gbase + x], (unsigned long long)v);
            }
    }
    flush_scalars(lsc, out.scalars + (size_t)J.group * NG_SCALARS, NG_SUMS, NG_MAXIMA, tid);
}

constexpr auto noma_gain_levels_kernel = &noma_columns_kernel<NomaGainLevels>;
template <int SCHEME> constexpr auto noma_gain_kernel = &noma_census_kernel<NomaGainUes, SCHEME>;

size_t noma_gain_lds_bytes(int scheme, int bins) { return 4 * (size_t)(TILE_SCHED_CAP + 2 * NG_SCALARS + (scheme == 1 ? 36 * bins : 0)); }

} // namespace

hipError_t launch_noma_gain_levels(const NomaGainJob *jobs, int njobs, int workgroups, unsigned *edges, int edge_cap, hipStream_t stream) {
    if (njobs < 1 || workgroups < 1 || !edges || edge_cap < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(noma_gain_levels_kernel, dim3(workgroups), dim3(TL_THREADS), 0, stream, jobs, njobs, edges, edge_cap);
    return hipGetLastError();
}

hipError_t launch_noma_gain_kernel(const NomaGainJob *jobs, int njobs, int workgroups, int bins, int width, int lo, int scheme, NomaGainOut out, hipStream_t stream) {
    if (bins < 1 || bins > PRACH_NOMA_GAIN_MAX_BINS || width < 1) return hipErrorInvalidValue;
    if (bins > NG_LDS_MAX_BINS) scheme = 0; // (the counters of a tile no longer fit beside a second workgroup's)
    const size_t lds = noma_gain_lds_bytes(scheme, bins);
    if (scheme == 0) return launch_with_lds(noma_gain_kernel<0>, workgroups, TL_THREADS, lds, stream, jobs, njobs, bins, width, lo, out);
    return launch_with_lds(noma_gain_kernel<1>, workgroups, TL_THREADS, lds, stream, jobs, njobs, bins, width, lo, out);
}

} // namespace prach
