// prach_summary.hip — prach::summary_kernel: ONE row per TRIAL (prach_run_trials_summary) — arrived / successful / restarted UEs, the sums and maxima of
// the sojourn c(i) - a(i), of `timer` and of preambleTxCounter over the successful UEs, and EXACT order statistics of the three at up to
// PRACH_SUMMARY_MAX_Q levels — selected on the device from the 64-byte per-UE log records a simulation kernel writes there (words 0-3 idx, timer, active,
// txTime; word 11 preambleTxCounter; word 14 msg4Flag) and from the trial's arrival schedule.  gfx950 only.  prach_summary_from_logs (prach_host.c) is the
// definition; this kernel equals it integer for integer.
//
// The jobs are the timeline's (TimelineJob, group = the row).  ONE workgroup per trial: a row is written with plain stores, nothing is shared between
// trials, so a trial that is rerun needs no subtraction (only the launch that is accepted has a job for it).  Two-level radix selection, values 0 .. 65 535:
//   pass 1  reads every record, counts, sums (64 bits) and maximises, and fills one LDS histogram per quantity of value >> 6 (1024 32-bit bins: a trial
//           has at most 2^24 UEs);
//   scan    per (quantity, level) target one wavefront scans that histogram (16 bins per lane, wave_scan_incl of prach_device_fn.h) for the coarse bin
//           holding rank r = max(1, (n m + 999) / 1000) and for the rank left inside it;
//   pass 2  reads the records again and adds value & 63 of the UEs inside a target's coarse bin to that target's 64-bin fine histogram (targets of one
//           quantity in one coarse bin share the first one's);
//   the value is coarse << 6 | fine bin reaching the rank left.
// A successful UE's value outside 0 .. 65 535 enters no histogram and is counted in the row's range errors (the engine voids that quantity's levels and
// fails the call).  No trial produces one: the sojourn is at most TL_MAX_SOJOURN, `timer` at most the same (it is a stretch of one UE's sojourn, the
// timeline's own bound), and preambleTxCounter is set to 1 or grows by at most one per subframe (prach_ue_body.h: ptc_set1 / ptc_inc, one event per UE
// and subframe), of which a trial has at most 60 000 + 6.  Integers only: the result does not depend on any order.
#include "prach_menu_body.h"

namespace prach {

namespace {

static_assert(TL_MAX_SOJOURN < 65536, "every sojourn and timer a trial can produce is inside the range the two-level selection ranks");
constexpr int SM_COARSE = SEL_COARSE, SM_FINE = SEL_FINE, SM_TARGETS = 3 * PRACH_SUMMARY_MAX_Q; // (the selection's steps and its two sizes: prach_menu_body.h)
constexpr int SM_SCHED_CAP = 12288; // schedule entries staged in LDS: Uniform traffic at accessTime 5 has 12 002 (a longer schedule is searched in global memory)
// LDS words: 3 coarse histograms | the fine histograms | 9 x 64-bit scalars (+ pad) | 3 maxima | per target: coarse bin, rank left, fine histogram used | schedule
constexpr int SM_FIXED_WORDS = 3 * SM_COARSE + SM_TARGETS * SM_FINE + 2 * 10 + 4 + 3 * SM_TARGETS; // 18.4 KB
static_assert(4 * (SM_FIXED_WORDS + SM_SCHED_CAP) <= 80 * 1024, "two workgroups per CU also with the longest staged schedule");

template <int THREADS>
__global__ __launch_bounds__(THREADS) void summary_kernel(const TimelineJob *__restrict__ jobs, int njobs, SummaryLevels lv, int scap, unsigned long long *__restrict__ rows) {
    extern __shared__ unsigned lds[]; // SM_FIXED_WORDS | [scap] schedule
    unsigned *const lcoarse = lds;
    unsigned *const lfine = lcoarse + 3 * SM_COARSE;
    long long *const lsc = reinterpret_cast<long long *>(lfine + SM_TARGETS * SM_FINE); // arrived, success, restarted, 3 range errors, 3 sums (8-byte aligned: even offset)
    int *const lmax = reinterpret_cast<int *>(lsc + 10);
    int *const tcoarse = lmax + 4;
    unsigned *const trem = reinterpret_cast<unsigned *>(tcoarse + SM_TARGETS);
    int *const tslot = reinterpret_cast<int *>(trem + SM_TARGETS);
    int *const lsched = tslot + SM_TARGETS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= njobs) return;
    const TimelineJob J = jobs[blockIdx.x];

    for (int w = tid; w < 3 * SM_COARSE + SM_TARGETS * SM_FINE; w += THREADS) lds[w] = 0;
    if (tid < 10) lsc[tid] = 0;
    if (tid < 3) lmax[tid] = -1;
    if (tid < SM_TARGETS) { tcoarse[tid] = -1; trem[tid] = 0; tslot[tid] = -1; }
    const bool staged = J.nslots <= scap;
    if (staged)
        for (int s = tid; s < J.nslots; s += THREADS) lsched[s] = J.sched[s];
    const int *const sp = staged ? lsched : J.sched;
    __syncthreads();

    // pass 1
    {
        int arrived = 0, nsucc = 0, nrest = 0, rerr0 = 0, rerr1 = 0, rerr2 = 0, max0 = -1, max1 = -1, max2 = -1;
        long long sum0 = 0, sum1 = 0, sum2 = 0;
        for (int i = tid; i < J.nUE; i += THREADS) {
            const int4 head = J.logs[4 * (size_t)i]; // idx, timer, active, txTime
            if (head.z == -1) continue;              // not arrived
            arrived++;
            if (J.logs[4 * (size_t)i + 3].z != 1) continue; // msg4Flag
            const int ptc = J.logs[4 * (size_t)i + 2].w;    // preambleTxCounter
            const int a = J.aT * first_slot_above(sp, 0, 0, J.nslots, i);
            const int c = head.w + 6, soj = c - a, timer = head.y;
            nsucc++;
            nrest += c - timer != a;
            sum0 += soj; sum1 += timer; sum2 += ptc;
            max0 = max(max0, soj); max1 = max(max1, timer); max2 = max(max2, ptc);
            if ((unsigned)soj <= (unsigned)SM_MAX_VALUE) atomicAdd(&lcoarse[(unsigned)soj >> 6], 1u); else rerr0++;
            if ((unsigned)timer <= (unsigned)SM_MAX_VALUE) atomicAdd(&lcoarse[SM_COARSE + ((unsigned)timer >> 6)], 1u); else rerr1++;
            if ((unsigned)ptc <= (unsigned)SM_MAX_VALUE) atomicAdd(&lcoarse[2 * SM_COARSE + ((unsigned)ptc >> 6)], 1u); else rerr2++;
        }
        // (the folds of prach_reduce_tile.h, on signed values: a sum folds alike, a maximum may be -1)
        arrived = fold_sum(arrived); nsucc = fold_sum(nsucc); nrest = fold_sum(nrest); rerr0 = fold_sum(rerr0); rerr1 = fold_sum(rerr1); rerr2 = fold_sum(rerr2);
        sum0 = fold_sum(sum0); sum1 = fold_sum(sum1); sum2 = fold_sum(sum2); max0 = fold_max(max0); max1 = fold_max(max1); max2 = fold_max(max2);
        if (lane == 0 && arrived) {
            unsigned long long *const u = reinterpret_cast<unsigned long long *>(lsc);
            atomicAdd(&u[0], (unsigned long long)arrived); atomicAdd(&u[1], (unsigned long long)nsucc); atomicAdd(&u[2], (unsigned long long)nrest);
            atomicAdd(&u[3], (unsigned long long)rerr0); atomicAdd(&u[4], (unsigned long long)rerr1); atomicAdd(&u[5], (unsigned long long)rerr2);
            atomicAdd(&u[6], (unsigned long long)sum0); atomicAdd(&u[7], (unsigned long long)sum1); atomicAdd(&u[8], (unsigned long long)sum2); // (two's complement: signed sums add up)
            atomicMax(&lmax[0], max0); atomicMax(&lmax[1], max1); atomicMax(&lmax[2], max2);
        }
    }
    __syncthreads();
    const long long n = lsc[1];

    // scan: target t = quantity * PRACH_SUMMARY_MAX_Q + level, one wavefront each (t is the same in every lane: all 64 lanes are in the DPP scan)
    if (n > 0)
        for (int t = wave; t < SM_TARGETS; t += THREADS / 64) {
            const int x = t / PRACH_SUMMARY_MAX_Q, l = t % PRACH_SUMMARY_MAX_Q;
            if (l >= lv.nq) continue;
            long long r = (n * (long long)lv.permille[l] + 999) / 1000;
            if (r < 1) r = 1;
            select_coarse(lcoarse + x * SM_COARSE, r, lane, &tcoarse[t], &trem[t]);
        }
    __syncthreads();
    select_fine_slots<SM_TARGETS>(tcoarse, tslot, tid);
    __syncthreads();

    // pass 2
    if (n > 0)
        for (int i = tid; i < J.nUE; i += THREADS) {
            const int4 head = J.logs[4 * (size_t)i];
            if (head.z == -1 || J.logs[4 * (size_t)i + 3].z != 1) continue;
            const int v[3] = {head.w + 6 - J.aT * first_slot_above(sp, 0, 0, J.nslots, i), head.y, J.logs[4 * (size_t)i + 2].w};
#pragma unroll
            for (int x = 0; x < 3; x++) {
                if ((unsigned)v[x] > (unsigned)SM_MAX_VALUE) continue;
                const int cb = (int)((unsigned)v[x] >> 6);
                for (int l = 0; l < lv.nq; l++) {
                    const int t = x * PRACH_SUMMARY_MAX_Q + l;
                    if (tcoarse[t] == cb && tslot[t] == t) atomicAdd(&lfine[t * SM_FINE + (v[x] & (SM_FINE - 1))], 1u);
                }
            }
        }
    __syncthreads();

    // the row: SM_WORDS 64-bit words (prach_device.h)
    unsigned long long *const row = rows + (size_t)J.group * SM_WORDS;
    if (tid < 9) row[tid] = (unsigned long long)lsc[tid];
    if (tid >= 9 && tid < 12) row[tid] = (unsigned long long)(long long)(n > 0 ? lmax[tid - 9] : -1);
    if (tid < SM_TARGETS) row[12 + tid] = (unsigned long long)select_level(lfine, tcoarse, trem, tslot, tid);
}

} // namespace

int summary_sched_cap() { return SM_SCHED_CAP; }

hipError_t launch_summary_kernel(const TimelineJob *jobs, int njobs, SummaryLevels levels, int threads, int sched_cap, unsigned long long *rows, hipStream_t stream) {
    if (sched_cap < 0 || sched_cap > SM_SCHED_CAP || levels.nq < 1 || levels.nq > PRACH_SUMMARY_MAX_Q) return hipErrorInvalidValue;
    const size_t lds = 4 * ((size_t)SM_FIXED_WORDS + (size_t)sched_cap);
    if (threads == 512) return launch_with_lds(summary_kernel<512>, njobs, 512, lds, stream, jobs, njobs, levels, sched_cap, rows);
    return launch_with_lds(summary_kernel<1024>, njobs, 1024, lds, stream, jobs, njobs, levels, sched_cap, rows);
}

} // namespace prach
