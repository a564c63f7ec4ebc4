// prach_noma_select.hip — the two per-trial selections over THE NOMA MENU of include/prach.h, made on the device from the 64-byte per-UE log records
// prach::noma_kernel writes there, the trial's arrival schedule and its `steps`.  gfx950 only.
//   prach::noma_summary_kernel  ONE row per TRIAL (prach_run_trials_noma_summary): the four class counts, `restarted`, and for up to four named menu fields over
//                               the UEs of the classes in `who` whose value is defined, their number, sum, maximum and EXACT order statistics at up to
//                               PRACH_SUMMARY_MAX_Q levels; prach_noma_summary_from_logs (prach_host.c) is the definition
//   prach::noma_pick_kernel     per TRIAL (prach_run_trials_noma_pick) the k UEs that match a predicate over the menu — the first k by UE index, or the k with
//                               the largest / smallest value of one menu field, equal keys in ascending UE index — as 80-byte records (prach_pick_row), and the
//                               exact number of matches; prach_noma_pick_from_logs is the definition
// Both equal their definition integer for integer.  They have the shape of prach::summary_kernel and prach::pick_kernel (prach_summary.hip, prach_pick.hip) and
// share what those share (prach_reduce_tile.h: the jobs, the slot search, the folds; the launch helper; SM_MAX_VALUE); the menu is prach_noma_menu.h.
// The SUMMARY keeps its own pass 1, pass 2 and row — its quantities are named by the caller where summary_kernel has three fixed ones, and the rows differ —
// and shares the three steps around them with summary_kernel: select_coarse, select_fine_slots, select_level of prach_menu_body.h.
// The PICK is a body of its own next to pick_kernel's, and that is a measured decision, not the mangled names (a __global__ function can keep its name and
// call a shared body, as the census and the columns kernels do): as one pick_body<Menu, THREADS> both picks ran 1.4 - 6.7 % slower on keyed picks, beyond the
// spread of the probes.  The compiler loads every word of the 72-byte spec at the kernel's entry when the spec reaches the body through a reference, where
// the kernels here read them from the kernel arguments at their uses, and these kernels already sit at the SGPR limit (profiles/menu_bodies.md 2).
//
// The jobs are the timeline's with E = min(steps, maxTime) in `pad` (TimelineJob, group = the trial; E from steps_of(), as for the census).  ONE workgroup per
// trial: rows and scalars are written with plain stores, nothing is shared between trials, so a trial that is rerun needs no subtraction (only the launch that
// is accepted has a job for it).  No atomics on global memory, integers only: the result does not depend on any order.
// LOADS, 16 bytes each: a lane reads words 8-11 (preambleChange = the sector, maxRarCounter, preambleTxCounter) and 12-15 (connectionRequest, msg4Flag,
// failCount) of a record always: the class needs them.  Words 0-3 and 4-7 only where a field, a clause or the key needs them (nm_needs_q0, nm_needs_q1), and
// the schedule (staged in LDS when it has at most NS_SCHED_CAP entries, searched in global memory beyond) only where one needs a(i) (nm_needs_arrival): all
// uniform for the launch.  The summary always has one such field: LOST stands behind `restarted`, so it reads words 0-3 and searches the schedule in every
// launch, and a pass of it moves 48 or 64 bytes per UE; a pass of the pick moves 32, 48 or 64.
//
// SUMMARY: two-level radix selection, values 0 .. 65 535, per named field x:
//   pass 1  reads every record, classifies and counts; over the selected UEs with a defined value of field x it counts (n[x]), sums (64 bits) and maximises,
//           and fills the field's LDS histogram of value >> 6 (1024 32-bit bins: a trial has at most 2^24 UEs);
//   scan    per (field, level) target one wavefront scans that histogram (16 bins per lane, wave_scan_incl of prach_device_fn.h) for the coarse bin holding
//           rank r = max(1, (n[x] m + 999) / 1000) and for the rank left inside it;
//   pass 2  reads the records again and adds value & 63 of the UEs inside a target's coarse bin to that target's 64-bin fine histogram (targets of one field
//           in one coarse bin share the first one's);
//   the value is coarse << 6 | fine bin reaching the rank left.
// A defined value outside 0 .. 65 535 enters n, sum and max, no histogram, and the row's range errors of its field (the engine voids that field's levels
// and fails the call).
//
// PICK, OUTPUT ORDER: the kernel leaves a trial's rows in UE-INDEX order (that is what an ordered compaction gives); the engine's unpack sorts the at most k
// rows of a trial into the defined order on the host (a stable sort by key).  WHICH rows are stored, and every count, is decided here.  The workgroup walks
// the UEs in blocks of THREADS consecutive indices, in up to three passes.
//   pass 1     classifies, evaluates the clauses and the key (nm_class, nm_value: the one statement of the menu) and counts selected, matched and undefined.
//              BY_INDEX: the ordered compaction below is fused into this pass, with the one flag `matched`.  LARGEST / SMALLEST: the RANK KEY — the key, or
//              65 535 - key under SMALLEST, so that the rows wanted are always the largest — enters a 1024-bin LDS histogram of rank key >> 6; a match with
//              a key outside 0 .. 65 535 enters nothing and is counted as a range error (the engine voids the trial's rows).
//   threshold  only when more than k matches are ranked: one wavefront scans the coarse histogram from the top (16 bins per lane, wave_scan_incl of
//              prach_device_fn.h) for the bin in which the count reaches k; pass 2 reads the records again and fills the 64-bin fine histogram of that
//              coarse bin; one lane walks it from the top.  That gives the threshold T, the number of rank keys above it and the k - above ties to take.
//              With at most k ranked matches T = -1: every one is above it.
//   pass 3     the ordered compaction.  Per block of THREADS UEs: a ballot and a popcount per wavefront for the two flags (rank key > T, rank key == T),
//              the per-wavefront totals in LDS (two copies, by block parity: one barrier per block), a running base in registers.  A UE's slot is
//              (rank keys above T before it) + min(ties before it, ties to take); a tie is stored iff its rank among the ties is below the number to
//              take.  A stored lane copies its 64-byte record, a(i) (-1: idle) and its key to its row with five 16-byte stores.
// THE BOUNDS (prach_noma_menu.h): no trial produces a key outside the range.  Bounded by the 10 000 + 6 subframes of a NOMA.c trial: ARRIVAL, COMPLETION and
// AGE (subframe numbers), SOJOURN and LOST (differences of two).  Logged words: TIMER (one tick per subframe), PTC and RETX (at most one per subframe),
// PREAMBLE (one of at most 64), SECTOR (0..5), MSG3FAIL (the upper half of failCount, at most one per subframe).  STATE is at most 8, ONE is 0.  A logged word
// the simulation did not write can be anything: above 65 535 it is a range error, negative it is UNDEFINED.
// The class and clause tests are selects on compares and products of 0 / 1 flags, as in the census kernels.
#include "prach_menu_body.h"
#include "prach_noma_menu.h"

namespace prach {

namespace {

constexpr int NS_COARSE = SEL_COARSE, NS_FINE = SEL_FINE, NS_MAX_KEY = SM_MAX_VALUE; // (the selection's two sizes: prach_menu_body.h)
static_assert(NS_COARSE == SEL_COARSE && NS_FINE == SEL_FINE && 10000 + 6 <= NS_MAX_KEY, "coarse << 6 | fine covers every key a trial produces; a wavefront scans the histogram in one go");
constexpr int NS_SCHED_CAP = 12288; // schedule entries staged in LDS: pick_kernel's cap (a NOMA.c trial has at most 10 000; a longer schedule is searched in global memory)
// the pick's layout (its kernel stands behind the summary's)
constexpr int NS_MAX_WAVES = 16;
// LDS words: coarse histogram | fine histogram | 2 copies x [NS_MAX_WAVES] x 2 per-wavefront totals | 16 scalars | schedule
constexpr int NS_FIXED_WORDS = NS_COARSE + NS_FINE + 4 * NS_MAX_WAVES + 16; // 4.6 KB
static_assert(4 * (NS_FIXED_WORDS + NS_SCHED_CAP) <= 80 * 1024 && NS_FIXED_WORDS % 4 == 0, "two workgroups per CU also with the longest staged schedule");
enum { L_SEL, L_MATCH, L_UNDEF, L_RERR, L_MINRK, L_CB, L_LEFT, L_T, L_TAKE, L_TIESOUT }; // the scalars

// ---- the summary ----------------------------------------------------------------------------------------------------------------------------------------
constexpr int NSM_FIELDS = PRACH_NOMA_SUMMARY_MAX_FIELDS, NSM_TARGETS = NSM_FIELDS * PRACH_SUMMARY_MAX_Q;
// LDS words: 4 coarse histograms | 32 fine histograms | 22 x 64-bit scalars (the last 4: the maxima) | per target: coarse bin, rank left, fine histogram used | schedule
constexpr int NSM_FIXED_WORDS = NSM_FIELDS * NS_COARSE + NSM_TARGETS * NS_FINE + 2 * 22 + 3 * NSM_TARGETS; // 25.1 KB
static_assert(NSM_FIELDS * NS_COARSE + NSM_TARGETS * NS_FINE == 4 * 1024 + 32 * 64, "the histograms of four fields and 32 (field, level) targets");
static_assert(4 * (NSM_FIXED_WORDS + NS_SCHED_CAP) <= 80 * 1024 && NSM_FIXED_WORDS % 2 == 0, "two workgroups per CU also with the longest staged schedule");
enum { S_IDLE, S_SERVED, S_DROPPED, S_PENDING, S_SEL, S_REST, S_RERR, S_N = S_RERR + NSM_FIELDS, S_SUM = S_N + NSM_FIELDS, S_MAX = S_SUM + NSM_FIELDS, S_END = S_MAX + NSM_FIELDS }; // the 64-bit scalars
static_assert(S_END == 22 && NSM_WORDS == S_END + NSM_TARGETS, "a row is the scalars, the maxima among them, and the levels (prach_device.h)");

template <int THREADS>
__global__ __launch_bounds__(THREADS) void noma_summary_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_noma_summary_spec sp, int scap, unsigned long long *__restrict__ rows) {
    extern __shared__ unsigned lds[]; // NSM_FIXED_WORDS | [scap] schedule
    unsigned *const lcoarse = lds;
    unsigned *const lfine = lcoarse + NSM_FIELDS * NS_COARSE;
    long long *const lsc = reinterpret_cast<long long *>(lfine + NSM_TARGETS * NS_FINE); // (8-byte aligned: an even offset)
    int *const tcoarse = reinterpret_cast<int *>(lsc + S_END);
    unsigned *const trem = reinterpret_cast<unsigned *>(tcoarse + NSM_TARGETS);
    int *const tslot = reinterpret_cast<int *>(trem + NSM_TARGETS);
    int *const lsched = tslot + NSM_TARGETS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= njobs) return;
    const TimelineJob J = jobs[blockIdx.x];
    const int E = J.pad;

    bool need_q1 = false; // (words 0-3 and a(i) are needed in every launch: LOST stands behind `restarted`)
#pragma unroll
    for (int x = 0; x < NSM_FIELDS; x++)
        if (x < sp.nfields) need_q1 |= nm_needs_q1(sp.field[x]);

    for (int w = tid; w < NSM_FIELDS * NS_COARSE + NSM_TARGETS * NS_FINE; w += THREADS) lds[w] = 0;
    if (tid < S_END) lsc[tid] = tid >= S_MAX ? -1 : 0;
    if (tid < NSM_TARGETS) { tcoarse[tid] = -1; trem[tid] = 0; tslot[tid] = -1; }
    const bool staged = J.nslots <= scap;
    if (staged)
        for (int s = tid; s < J.nslots; s += THREADS) lsched[s] = J.sched[s];
    const int *const schedp = staged ? lsched : J.sched;
    __syncthreads();

    // pass 1
    {
        int nidle = 0, nserved = 0, ndropped = 0, npending = 0, nsel = 0, nrest = 0;
        int cnt[NSM_FIELDS] = {0, 0, 0, 0}, rerr[NSM_FIELDS] = {0, 0, 0, 0};
        long long sum[NSM_FIELDS] = {0, 0, 0, 0}, mx[NSM_FIELDS] = {-1, -1, -1, -1};
        for (int i = tid; i < J.nUE; i += THREADS) {
            const int4 q0 = J.logs[4 * (size_t)i]; // idx, timer, active, txTime
            int4 q1 = make_int4(0, 0, 0, 0);
            if (need_q1) q1 = J.logs[4 * (size_t)i + 1]; // firstTxTime, secondTxTime, nowBackoff, preamble
            const int4 q2 = J.logs[4 * (size_t)i + 2];   // preambleChange (sector), rarWindow, maxRarCounter, preambleTxCounter
            const int4 q3 = J.logs[4 * (size_t)i + 3];   // msg2Flag, connectionRequest, msg4Flag, failCount
            const int cls = nm_class(q2, q3);
            nidle += cls == PRACH_NOMA_IDLE; nserved += cls == PRACH_NOMA_SERVED; ndropped += cls == PRACH_NOMA_DROPPED; npending += cls == PRACH_NOMA_PENDING;
            const int a = J.aT * first_slot_above(schedp, 0, 0, J.nslots, i);
            nrest += nm_value(PRACH_NOMA_LOST, q0, q1, q2, q3, cls, a, E) > 0; // (defined for the served only)
            if (!(sp.who & cls)) continue;
            nsel++;
#pragma unroll
            for (int x = 0; x < NSM_FIELDS; x++)
                if (x < sp.nfields) {
                    const long long v = nm_value(sp.field[x], q0, q1, q2, q3, cls, a, E);
                    if (v < 0) continue; // UNDEFINED
                    cnt[x]++; sum[x] += v; mx[x] = max(mx[x], v);
                    if (v <= (long long)NS_MAX_KEY) atomicAdd(&lcoarse[x * NS_COARSE + (int)(v >> 6)], 1u); else rerr[x]++;
                }
        }
        nidle = fold_sum(nidle); nserved = fold_sum(nserved); ndropped = fold_sum(ndropped); npending = fold_sum(npending); nsel = fold_sum(nsel); nrest = fold_sum(nrest);
#pragma unroll
        for (int x = 0; x < NSM_FIELDS; x++) { cnt[x] = fold_sum(cnt[x]); rerr[x] = fold_sum(rerr[x]); sum[x] = fold_sum(sum[x]); mx[x] = fold_max(mx[x]); }
        if (lane == 0) {
            unsigned long long *const u = reinterpret_cast<unsigned long long *>(lsc);
            atomicAdd(&u[S_IDLE], (unsigned long long)nidle); atomicAdd(&u[S_SERVED], (unsigned long long)nserved); atomicAdd(&u[S_DROPPED], (unsigned long long)ndropped);
            atomicAdd(&u[S_PENDING], (unsigned long long)npending); atomicAdd(&u[S_SEL], (unsigned long long)nsel); atomicAdd(&u[S_REST], (unsigned long long)nrest);
#pragma unroll
            for (int x = 0; x < NSM_FIELDS; x++) {
                atomicAdd(&u[S_RERR + x], (unsigned long long)rerr[x]); atomicAdd(&u[S_N + x], (unsigned long long)cnt[x]); atomicAdd(&u[S_SUM + x], (unsigned long long)sum[x]);
                atomicMax(&lsc[S_MAX + x], mx[x]); // (64 bits: a menu value is below 2^31 + 6; -1 where nothing is defined)
            }
        }
    }
    __syncthreads();

    // scan: target t = field * PRACH_SUMMARY_MAX_Q + level, one wavefront each (t is the same in every lane: all 64 lanes are in the DPP scan)
    for (int t = wave; t < NSM_TARGETS; t += THREADS / 64) {
        const int x = t / PRACH_SUMMARY_MAX_Q, l = t % PRACH_SUMMARY_MAX_Q;
        const long long n = lsc[S_N + x];
        if (x >= sp.nfields || l >= sp.nq || n <= 0) continue;
        long long r = (n * (long long)sp.permille[l] + 999) / 1000;
        if (r < 1) r = 1;
        select_coarse(lcoarse + x * NS_COARSE, r, lane, &tcoarse[t], &trem[t]);
    }
    __syncthreads();
    select_fine_slots<NSM_TARGETS>(tcoarse, tslot, tid);
    __syncthreads();

    // pass 2
    if (lsc[S_SEL] > 0)
        for (int i = tid; i < J.nUE; i += THREADS) {
            int4 q1 = make_int4(0, 0, 0, 0);
            if (need_q1) q1 = J.logs[4 * (size_t)i + 1];
            const int4 q2 = J.logs[4 * (size_t)i + 2];
            const int4 q3 = J.logs[4 * (size_t)i + 3];
            const int cls = nm_class(q2, q3);
            if (!(sp.who & cls)) continue;
            const int4 q0 = J.logs[4 * (size_t)i];
            const int a = J.aT * first_slot_above(schedp, 0, 0, J.nslots, i);
#pragma unroll
            for (int x = 0; x < NSM_FIELDS; x++)
                if (x < sp.nfields) {
                    const long long v = nm_value(sp.field[x], q0, q1, q2, q3, cls, a, E);
                    if ((unsigned long long)v > (unsigned long long)NS_MAX_KEY) continue; // undefined, or a range error
                    const int cb = (int)(v >> 6);
                    for (int l = 0; l < sp.nq; l++) {
                        const int t = x * PRACH_SUMMARY_MAX_Q + l;
                        if (tcoarse[t] == cb && tslot[t] == t) atomicAdd(&lfine[t * NS_FINE + ((int)v & (NS_FINE - 1))], 1u);
                    }
                }
        }
    __syncthreads();

    // the row: NSM_WORDS 64-bit words (prach_device.h)
    unsigned long long *const row = rows + (size_t)J.group * NSM_WORDS;
    if (tid < S_END) row[tid] = (unsigned long long)lsc[tid];
    if (tid < NSM_TARGETS) row[S_END + tid] = (unsigned long long)select_level(lfine, tcoarse, trem, tslot, tid);
}

// ---- the pick -------------------------------------------------------------------------------------------------------------------------------------------
struct NomaPickUe {
    int cls;               // the class bit, PRACH_NOMA_* (0: no UE)
    int sel, match, undef; // 0 / 1
    long long key;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void noma_pick_kernel(const TimelineJob *__restrict__ jobs, int njobs, prach_pick_spec sp, int scap, unsigned long long *__restrict__ rows,
                                                            unsigned long long *__restrict__ scalars) {
    constexpr int WAVES = THREADS / 64;
    static_assert(WAVES <= NS_MAX_WAVES, "the per-wavefront totals have room");
    extern __shared__ unsigned lds[]; // NS_FIXED_WORDS | [scap] schedule
    unsigned *const lcoarse = lds;
    unsigned *const lfine = lcoarse + NS_COARSE;
    int *const lwt = reinterpret_cast<int *>(lfine + NS_FINE);
    int *const lsc = lwt + 4 * NS_MAX_WAVES;
    int *const lsched = lsc + 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= njobs) return;
    const TimelineJob J = jobs[blockIdx.x];
    const int E = J.pad, k = sp.k;
    const bool keyed = sp.order != PRACH_PICK_BY_INDEX, largest = sp.order == PRACH_PICK_LARGEST;

    bool need_a = keyed && nm_needs_arrival(sp.key_field), need_q0 = keyed && nm_needs_q0(sp.key_field), need_q1 = keyed && nm_needs_q1(sp.key_field);
#pragma unroll
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++)
        if (c < sp.nclauses) { need_a |= nm_needs_arrival(sp.clause[c].field); need_q0 |= nm_needs_q0(sp.clause[c].field); need_q1 |= nm_needs_q1(sp.clause[c].field); }

    for (int w = tid; w < NS_COARSE + NS_FINE; w += THREADS) lds[w] = 0;
    if (tid < 16) lsc[tid] = tid == L_MINRK ? INT_MAX : 0;
    const bool staged = need_a && J.nslots <= scap; // (without a field that needs a(i) only the stored lanes search, in global memory)
    if (staged)
        for (int s = tid; s < J.nslots; s += THREADS) lsched[s] = J.sched[s];
    const int *const schedp = staged ? lsched : J.sched;
    __syncthreads();

    // one UE: its class, whether it is selected, matches, or is undefined, and its key (include/prach.h)
    auto eval = [&](int i) {
        NomaPickUe u;
        int4 q0 = make_int4(0, 0, 0, 0), q1 = make_int4(0, 0, 0, 0);
        if (need_q0) q0 = J.logs[4 * (size_t)i];     // idx, timer, active, txTime
        if (need_q1) q1 = J.logs[4 * (size_t)i + 1]; // firstTxTime, secondTxTime, nowBackoff, preamble
        const int4 q2 = J.logs[4 * (size_t)i + 2];   // preambleChange (sector), rarWindow, maxRarCounter, preambleTxCounter
        const int4 q3 = J.logs[4 * (size_t)i + 3];   // msg2Flag, connectionRequest, msg4Flag, failCount
        u.cls = nm_class(q2, q3);
        u.sel = (sp.who & u.cls) != 0;
        const int a = need_a ? J.aT * first_slot_above(schedp, 0, 0, J.nslots, i) : 0;
        int fails = 0, undef = 0;
#pragma unroll
        for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++)
            if (c < sp.nclauses) {
                const long long v = nm_value(sp.clause[c].field, q0, q1, q2, q3, u.cls, a, E);
                if (v < 0) undef = 1;
                else if (v < (long long)sp.clause[c].lo || v > (long long)sp.clause[c].hi) fails = 1;
            }
        u.key = keyed ? nm_value(sp.key_field, q0, q1, q2, q3, u.cls, a, E) : 0;
        if (u.key < 0) undef = 1;
        u.match = u.sel * (1 - fails) * (1 - undef);
        u.undef = u.sel * (1 - fails) * undef;
        return u;
    };
    // the ordered compaction of one block of THREADS consecutive UEs; EVERY thread of the workgroup calls (a barrier inside).  fa / fb: this lane's UE is
    // above the threshold / a tie on it.  Returns the lane's slot, -1 where its UE is not stored; base_a / base_b run on (the same in every thread)
    auto ordered = [&](bool fa, bool fb, int take, int &base_a, int &base_b, int blk) {
        const unsigned long long ba = __ballot(fa), bb = __ballot(fb), below = (1ull << lane) - 1ull;
        int *const wt = lwt + (blk & 1) * 2 * NS_MAX_WAVES; // (block n + 2 writes this copy again only behind the barrier of block n + 1, which every reader of block n has passed)
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
    auto store = [&](int slot, int i, const NomaPickUe &u) {
        if ((unsigned)slot >= (unsigned)k) return; // (never: a slot is below the number of rows to store)
        const int a = u.cls == PRACH_NOMA_IDLE ? -1 : J.aT * first_slot_above(schedp, 0, 0, J.nslots, i);
        int4 *const dst = myrows + 5 * (size_t)slot;
        dst[0] = J.logs[4 * (size_t)i]; dst[1] = J.logs[4 * (size_t)i + 1]; dst[2] = J.logs[4 * (size_t)i + 2]; dst[3] = J.logs[4 * (size_t)i + 3];
        dst[4] = make_int4(a, (int)u.key, 0, 0);
    };
    // the rank key of a match; -1: the key is outside the range that is ranked
    auto rank_key = [&](const NomaPickUe &u) { return (unsigned long long)u.key > (unsigned long long)NS_MAX_KEY ? -1 : largest ? (int)u.key : NS_MAX_KEY - (int)u.key; };

    // pass 1
    {
        int nsel = 0, nmat = 0, nund = 0, nerr = 0, minrk = INT_MAX, base_a = 0, base_b = 0;
        for (int base = 0, blk = 0; base < J.nUE; base += THREADS, blk++) {
            const int i = base + tid;
            NomaPickUe u{};
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
                const unsigned *const h = lcoarse + (NS_COARSE - 1) - lane * (NS_COARSE / 64);
                int s = 0;
#pragma unroll
                for (int b = 0; b < NS_COARSE / 64; b++) s += (int)*(h - b);
                const int incl = wave_scan_incl(s), excl = incl - s;
                if (excl < k && k <= incl) { // one lane
                    int left = k - excl, b = 0;
                    while (left > (int)*(h - b)) left -= (int)*(h - b++); // (ends inside the lane's bins: their sum s >= left)
                    lsc[L_CB] = (NS_COARSE - 1) - lane * (NS_COARSE / 64) - b;
                    lsc[L_LEFT] = left;
                }
            }
            __syncthreads();
            const int cb = lsc[L_CB];
            // pass 2
            for (int i = tid; i < J.nUE; i += THREADS) {
                const NomaPickUe u = eval(i);
                if (!u.match) continue;
                const int rk = rank_key(u);
                if (rk >= 0 && (rk >> 6) == cb) atomicAdd(&lfine[rk & (NS_FINE - 1)], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int left = lsc[L_LEFT], f = NS_FINE - 1;
                while (f > 0 && left > (int)lfine[f]) left -= (int)lfine[f--];
                lsc[L_T] = (cb << 6) | f;
                lsc[L_TAKE] = left;
                lsc[L_TIESOUT] = (int)lfine[f] - left;
            }
            __syncthreads();
            T = lsc[L_T]; take = lsc[L_TAKE]; ties_out = lsc[L_TIESOUT];
        }
        const int trk = ranked > k ? T : lsc[L_MINRK]; // the rank key of the last row in the defined order
        threshold = ranked == 0 ? -1 : largest ? trk : NS_MAX_KEY - trk;
        // pass 3
        int base_a = 0, base_b = 0;
        for (int base = 0, blk = 0; base < J.nUE; base += THREADS, blk++) {
            const int i = base + tid;
            NomaPickUe u{};
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

int noma_select_sched_cap() { return NS_SCHED_CAP; }

hipError_t launch_noma_summary_kernel(const TimelineJob *jobs, int njobs, prach_noma_summary_spec spec, int threads, int sched_cap, unsigned long long *rows, hipStream_t stream) {
    if (sched_cap < 0 || sched_cap > NS_SCHED_CAP || !prach_internal_noma_summary_spec_ok(&spec)) return hipErrorInvalidValue;
    const size_t lds = 4 * ((size_t)NSM_FIXED_WORDS + (size_t)sched_cap);
    if (threads == 512) return launch_with_lds(noma_summary_kernel<512>, njobs, 512, lds, stream, jobs, njobs, spec, sched_cap, rows);
    return launch_with_lds(noma_summary_kernel<1024>, njobs, 1024, lds, stream, jobs, njobs, spec, sched_cap, rows);
}

hipError_t launch_noma_pick_kernel(const TimelineJob *jobs, int njobs, prach_pick_spec spec, int threads, int sched_cap, unsigned long long *rows, unsigned long long *scalars,
                                   hipStream_t stream) {
    if (sched_cap < 0 || sched_cap > NS_SCHED_CAP || !prach_internal_noma_pick_spec_ok(&spec)) return hipErrorInvalidValue;
    const size_t lds = 4 * ((size_t)NS_FIXED_WORDS + (size_t)sched_cap);
    if (threads == 512) return launch_with_lds(noma_pick_kernel<512>, njobs, 512, lds, stream, jobs, njobs, spec, sched_cap, rows, scalars);
    return launch_with_lds(noma_pick_kernel<1024>, njobs, 1024, lds, stream, jobs, njobs, spec, sched_cap, rows, scalars);
}

} // namespace prach
