// prach_pick.hip — prach::pick_kernel: per TRIAL (prach_run_trials_pick) the k UEs that match a predicate over the menu of per-UE quantities of
// include/prach.h — the first k by UE index, or the k with the largest / smallest value of one menu field, equal keys in ascending UE index — as 80-byte
// records (prach_pick_row), and the exact number of matches, selected on the device from the 64-byte per-UE log records a simulation kernel writes there,
// the trial's arrival schedule and its `steps`.  gfx950 only.  prach_pick_from_logs (prach_host.c) is the definition.
//
// OUTPUT ORDER: the kernel leaves a trial's rows in UE-INDEX order (that is what an ordered compaction gives); the engine's unpack sorts the at most k
// rows of a trial into the defined order on the host (a stable sort by key).  WHICH rows are stored, and every count, is decided here.
//
// The jobs are the timeline's with E = min(steps, maxTime) in `pad` (TimelineJob, group = the trial).  ONE workgroup per trial, as prach::summary_kernel
// has and for its reason: rows and scalars are written with plain stores, nothing is shared between trials, so a trial that is rerun needs no subtraction
// (only the launch that is accepted has a job for it).  The workgroup walks the UEs in blocks of THREADS consecutive indices, in up to three passes.  A
// lane reads words 0-3 and 12-15 of a record always, words 4-7 (nowBackoff) only where a clause or the key is STATE, words 8-11 (preambleTxCounter) only
// where one is PTC, and searches the schedule (staged in LDS when it has at most PK_SCHED_CAP entries) only where one needs a(i): all uniform for the launch.
//   pass 1     classifies, evaluates the clauses and the key (xt_value of prach_xtab_menu.h: the one statement of the menu) and counts selected, matched
//              and undefined.  BY_INDEX: the ordered compaction below is fused into this pass, with the one flag `matched`.  LARGEST / SMALLEST: the RANK
//              KEY — the key, or 65 535 - key under SMALLEST, so that the rows wanted are always the largest — enters a 1024-bin LDS histogram of
//              rank key >> 6; a match with a key outside 0 .. 65 535 enters nothing and is counted as a range error (the engine voids the trial's rows).
//   threshold  only when more than k matches are ranked: one wavefront scans the coarse histogram from the top (16 bins per lane, wave_scan_incl of
//              prach_device_fn.h) for the bin in which the count reaches k; pass 2 reads the records again and fills the 64-bin fine histogram of that
//              coarse bin; one lane walks it from the top.  That gives the threshold T, the number of rank keys above it and the k - above ties to take.
//              With at most k ranked matches T = -1: every one is above it.
//   pass 3     the ordered compaction.  Per block of THREADS UEs: a ballot and a popcount per wavefront for the two flags (rank key > T, rank key == T),
//              the per-wavefront totals in LDS (two copies, by block parity: one barrier per block), a running base in registers.  A UE's slot is
//              (rank keys above T before it) + min(ties before it, ties to take); a tie is stored iff its rank among the ties is below the number to
//              take.  A stored lane copies its 64-byte record, a(i) (-1: idle) and its key to its row with five 16-byte stores.
// No trial produces a key outside the range: the sojourn is at most TL_MAX_SOJOURN and `timer` a stretch of it, preambleTxCounter grows by at most one per
// subframe (prach_summary.hip states the three); an arrival, a completion and an age are subframe numbers of a trial of at most 60 000 + 6; failCount grows
// by at most one per subframe; STATE is at most 6.  Integers only, and no atomics on global memory: the result does not depend on any order.
#include "prach_device.h"
#include "prach_device_fn.h"
#include "prach_reduce_tile.h"
#include "prach_xtab_menu.h"

namespace prach {

namespace {

constexpr int PK_COARSE = 1024, PK_FINE = 64, PK_MAX_KEY = SM_MAX_VALUE;
static_assert(PK_COARSE * PK_FINE == PK_MAX_KEY + 1 && PK_COARSE % 64 == 0 && TL_MAX_SOJOURN <= PK_MAX_KEY, "coarse << 6 | fine covers every key a trial produces; a wavefront scans the histogram in one go");
constexpr int PK_SCHED_CAP = 12288; // schedule entries staged in LDS: Uniform traffic at accessTime 5 has 12 002 (a longer schedule is searched in global memory)
constexpr int PK_MAX_WAVES = 16;
// LDS words: coarse histogram | fine histogram | 2 copies x [PK_MAX_WAVES] x 2 per-wavefront totals | 16 scalars | schedule
constexpr int PK_FIXED_WORDS = PK_COARSE + PK_FINE + 4 * PK_MAX_WAVES + 16; // 4.6 KB
static_assert(4 * (PK_FIXED_WORDS + PK_SCHED_CAP) <= 80 * 1024 && PK_FIXED_WORDS % 4 == 0, "two workgroups per CU also with the longest staged schedule");
enum { L_SEL, L_MATCH, L_UNDEF, L_RERR, L_MINRK, L_CB, L_LEFT, L_T, L_TAKE, L_TIESOUT }; // the scalars

struct PickUe {
    int4 head, tail;
    int cls;       // 0 idle, 1 served, 2 unserved
    int sel, match, undef; // 0 / 1
    long long key;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void pick_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_pick_spec sp, int scap, unsigned long long *__restrict__ rows,
                                                       unsigned long long *__restrict__ scalars) {
    constexpr int WAVES = THREADS / 64;
    static_assert(WAVES <= PK_MAX_WAVES, "the per-wavefront totals have room");
    extern __shared__ unsigned lds[]; // PK_FIXED_WORDS | [scap] schedule
    unsigned *const lcoarse = lds;
    unsigned *const lfine = lcoarse + PK_COARSE;
    int *const lwt = reinterpret_cast<int *>(lfine + PK_FINE);
    int *const lsc = lwt + 4 * PK_MAX_WAVES;
    int *const lsched = lsc + 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= njobs) return;
    const TimelineJob J = jobs[blockIdx.x];
    const int E = J.pad, k = sp.k;
    const bool keyed = sp.order != PRACH_PICK_BY_INDEX, largest = sp.order == PRACH_PICK_LARGEST;

    bool need_a = keyed && needs_arrival(sp.key_field), need_b = keyed && sp.key_field == PRACH_XTAB_STATE, need_p = keyed && sp.key_field == PRACH_XTAB_PTC;
#pragma unroll
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++)
        if (c < sp.nclauses) { need_a |= needs_arrival(sp.clause[c].field); need_b |= sp.clause[c].field == PRACH_XTAB_STATE; need_p |= sp.clause[c].field == PRACH_XTAB_PTC; }

    for (int w = tid; w < PK_COARSE + PK_FINE; w += THREADS) lds[w] = 0;
    if (tid < 16) lsc[tid] = tid == L_MINRK ? INT_MAX : 0;
    const bool staged = need_a && J.nslots <= scap; // (without a field that needs a(i) only the stored lanes search, in global memory)
    if (staged)
        for (int s = tid; s < J.nslots; s += THREADS) lsched[s] = J.sched[s];
    const int *const schedp = staged ? lsched : J.sched;
    __syncthreads();

    // one UE: its class, whether it is selected, matches, or is undefined, and its key (include/prach.h)
    auto eval = [&](int i) {
        PickUe u;
        u.head = J.logs[4 * (size_t)i];     // idx, timer, active, txTime
        u.tail = J.logs[4 * (size_t)i + 3]; // msg2Flag, connectionRequest, msg4Flag, failCount
        const int nowBackoff = need_b ? J.logs[4 * (size_t)i + 1].z : 0;
        const int ptc = need_p ? J.logs[4 * (size_t)i + 2].w : 0;
        u.cls = u.head.z == -1 ? 0 : u.tail.z == 1 ? 1 : 2;
        const int bit = u.cls == 0 ? PRACH_XTAB_IDLE : u.cls == 1 ? PRACH_XTAB_SERVED : PRACH_XTAB_UNSERVED;
        u.sel = (sp.who & bit) != 0;
        const int a = need_a ? J.aT * first_slot_above(schedp, 0, 0, J.nslots, i) : 0;
        int fails = 0, undef = 0;
#pragma unroll
        for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++)
            if (c < sp.nclauses) {
                const long long v = xt_value(sp.clause[c].field, u.head, u.tail, nowBackoff, ptc, u.cls, a, E);
                if (v < 0) undef = 1;
                else if (v < (long long)sp.clause[c].lo || v > (long long)sp.clause[c].hi) fails = 1;
            }
        u.key = keyed ? xt_value(sp.key_field, u.head, u.tail, nowBackoff, ptc, u.cls, a, E) : 0;
        if (u.key < 0) undef = 1;
        u.match = u.sel * (1 - fails) * (1 - undef);
        u.undef = u.sel * (1 - fails) * undef;
        return u;
    };
    // the ordered compaction of one block of THREADS consecutive UEs; EVERY thread of the workgroup calls (a barrier inside).  fa / fb: this lane's UE is
    // above the threshold / a tie on it.  Returns the lane's slot, -1 where its UE is not stored; base_a / base_b run on (the same in every thread)
    auto ordered = [&](bool fa, bool fb, int take, int &base_a, int &base_b, int blk) {
        const unsigned long long ba = __ballot(fa), bb = __ballot(fb), below = (1ull << lane) - 1ull;
        int *const wt = lwt + (blk & 1) * 2 * PK_MAX_WAVES; // (block n + 2 writes this copy again only behind the barrier of block n + 1, which every reader of block n has passed)
        if (lane == 0) { wt[2 * wave] = __popcll(ba); wt[2 * wave + 1] = __popcll(bb); }
        __syncthreads();
        int pa = base_a + __popcll(ba & below), pb = base_b + __popcll(bb & below);
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const int xa = wt[2 * w], xb = wt[2 * w + 1];
            base_a += xa; base_b += xb;
            if (w < wave) { pa += xa; pb += xb; }
        }
        return fa || (fb && pb < take) ? pa + min(pb, take) : -1;
    };
    int4 *const myrows = reinterpret_cast<int4 *>(rows + (size_t)J.group * (size_t)k * PK_ROW_WORDS);
    auto store = [&](int slot, int i, const PickUe &u) {
        if ((unsigned)slot >= (unsigned)k) return; // (never: a slot is below the number of rows to store)
        const int a = u.cls == 0 ? -1 : J.aT * first_slot_above(schedp, 0, 0, J.nslots, i);
        int4 *const dst = myrows + 5 * (size_t)slot;
        dst[0] = u.head; dst[1] = J.logs[4 * (size_t)i + 1]; dst[2] = J.logs[4 * (size_t)i + 2]; dst[3] = u.tail;
        dst[4] = make_int4(a, (int)u.key, 0, 0);
    };
    // the rank key of a match; -1: the key is outside the range that is ranked
    auto rank_key = [&](const PickUe &u) { return (unsigned long long)u.key > (unsigned long long)PK_MAX_KEY ? -1 : largest ? (int)u.key : PK_MAX_KEY - (int)u.key; };

    // pass 1
    {
        int nsel = 0, nmat = 0, nund = 0, nerr = 0, minrk = INT_MAX, base_a = 0, base_b = 0;
        for (int base = 0, blk = 0; base < J.nUE; base += THREADS, blk++) {
            const int i = base + tid;
            PickUe u{};
            if (i < J.nUE) u = eval(i);
            nsel += u.sel; nmat += u.match; nund += u.undef;
            if (!keyed) {
                const int slot = ordered(u.match != 0, false, 0, base_a, base_b, blk);
                if (slot >= 0) store(slot, i, u);
            } else if (u.match) {
                const int rk = rank_key(u);
                if (rk >= 0) { atomicAdd(&lcoarse[rk >> 6], 1u); minrk = min(minrk, rk); } else nerr++;
            }
        }
        nsel = fold_sum(nsel); nmat = fold_sum(nmat); nund = fold_sum(nund); nerr = fold_sum(nerr); minrk = -fold_max(-minrk);
        if (lane == 0) {
            atomicAdd(&lsc[L_SEL], nsel); atomicAdd(&lsc[L_MATCH], nmat); atomicAdd(&lsc[L_UNDEF], nund); atomicAdd(&lsc[L_RERR], nerr);
            atomicMin(&lsc[L_MINRK], minrk);
        }
    }
    __syncthreads();
    const int nselected = lsc[L_SEL], nmatched = lsc[L_MATCH], nundefined = lsc[L_UNDEF], nerrors = lsc[L_RERR];
    const int ranked = nmatched - nerrors; // the matches in the histogram (BY_INDEX: all of them)
    int T = -1, take = 0, threshold = -1, ties_out = 0;

    if (keyed) {
        if (ranked > k) {
            // threshold: lane l scans the bins 1023 - 16 l downwards (all 64 lanes of wavefront 0 are in the DPP scan)
            if (wave == 0) {
                const unsigned *const h = lcoarse + (PK_COARSE - 1) - lane * (PK_COARSE / 64);
                int s = 0;
#pragma unroll
                for (int b = 0; b < PK_COARSE / 64; b++) s += (int)*(h - b);
                const int incl = wave_scan_incl(s), excl = incl - s;
                if (excl < k && k <= incl) { // one lane
                    int left = k - excl, b = 0;
                    while (left > (int)*(h - b)) left -= (int)*(h - b++); // (ends inside the lane's bins: their sum s >= left)
                    lsc[L_CB] = (PK_COARSE - 1) - lane * (PK_COARSE / 64) - b;
                    lsc[L_LEFT] = left;
                }
            }
            __syncthreads();
            const int cb = lsc[L_CB];
            // pass 2
            for (int i = tid; i < J.nUE; i += THREADS) {
                const PickUe u = eval(i);
                if (!u.match) continue;
                const int rk = rank_key(u);
                if (rk >= 0 && (rk >> 6) == cb) atomicAdd(&lfine[rk & (PK_FINE - 1)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int left = lsc[L_LEFT], f = PK_FINE - 1;
                while (f > 0 && left > (int)lfine[f]) left -= (int)lfine[f--];
                lsc[L_T] = (cb << 6) | f;
                lsc[L_TAKE] = left;
                lsc[L_TIESOUT] = (int)lfine[f] - left;
            }
            __syncthreads();
            T = lsc[L_T]; take = lsc[L_TAKE]; ties_out = lsc[L_TIESOUT];
        }
        const int trk = ranked > k ? T : lsc[L_MINRK]; // the rank key of the last row in the defined order
        threshold = ranked == 0 ? -1 : largest ? trk : PK_MAX_KEY - trk;
        // pass 3
        int base_a = 0, base_b = 0;
        for (int base = 0, blk = 0; base < J.nUE; base += THREADS, blk++) {
            const int i = base + tid;
            PickUe u{};
            int rk = -1;
            if (i < J.nUE) { u = eval(i); if (u.match) rk = rank_key(u); }
            const int slot = ordered(rk > T, rk >= 0 && rk == T, take, base_a, base_b, blk);
            if (slot >= 0) store(slot, i, u);
        }
    }

    if (tid == 0) { // PK_SCALARS words (prach_device.h)
        long long *const q = reinterpret_cast<long long *>(scalars) + (size_t)J.group * PK_SCALARS;
        q[0] = nselected; q[1] = nmatched; q[2] = min(ranked, k); q[3] = nundefined; q[4] = nerrors; q[5] = threshold; q[6] = ties_out; q[7] = 0;
    }
}

} // namespace

int pick_sched_cap() { return PK_SCHED_CAP; }

hipError_t launch_pick_kernel(const TimelineJob *jobs, int njobs, prach_pick_spec spec, int threads, int sched_cap, unsigned long long *rows, unsigned long long *scalars,
                              hipStream_t stream) {
    if (sched_cap < 0 || sched_cap > PK_SCHED_CAP || !prach_internal_pick_spec_ok(&spec)) return hipErrorInvalidValue;
    const size_t lds = 4 * ((size_t)PK_FIXED_WORDS + (size_t)sched_cap);
    if (threads == 512) return launch_with_lds(pick_kernel<512>, njobs, 512, lds, stream, jobs, njobs, spec, sched_cap, rows, scalars);
    return launch_with_lds(pick_kernel<1024>, njobs, 1024, lds, stream, jobs, njobs, spec, sched_cap, rows, scalars);
}

} // namespace prach
