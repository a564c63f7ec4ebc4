// prach_device.h — device-side data layout shared by the kernels (prach_kernels.hip) and the
// engine (prach_engine.hip).  gfx950 (MI355X / CDNA4) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/prach.h"

namespace prach {

// ---- per-UE hot record: ONE 16-byte word (a single global_load_dwordx4 per UE per subframe) -------
//   x  txTime                       (Beta.c:15)   [PEND_RESET: the drawn backoff `tmp`, until applied]
//   y  tb  timer base: the subframe at which `timer` was last zeroed (timer = executed - tb), or the
//          final timer value once the UE has succeeded (Beta.c:13,378)
//   z  bo  nowBackoff, stored as its expiry subframe when positive (value = max(bo - t, 0)), as the
//          literal value when <= 0 (Beta.c:25)     [PEND_RESET: the UE's previous preamble]
//   w  pk  packed small fields, see below
// timer and nowBackoff are therefore never rewritten while a UE merely waits (timerIncrease,
// Beta.c:413-419, costs no memory traffic).
constexpr unsigned PK_ACT_SHIFT = 0, PK_CONN_SHIFT = 2, PK_PRE_SHIFT = 4, PK_RAR_SHIFT = 12, PK_MRC_SHIFT = 20,
                   PK_PEND_SHIFT = 28;
constexpr int ACT_IDLE = 0; // active == -1 (not yet arrived)
constexpr int ACT_DONE = 1; // active ==  0 (msg4Flag == 1)
constexpr int ACT_M1 = 2;   // active ==  1 (Msg1/Msg2 phase)
constexpr int ACT_M3 = 3;   // active ==  2 (Msg3/Msg4 phase)

// what the deferred "apply" of the previous subframe still owes this UE
constexpr int PEND_NONE = 0, PEND_STAY = 1, PEND_CALLER = 2, PEND_RESET = 3, PEND_PASSIVE = 4, PEND_RJOIN = 5;
// bit 31 of the packed word: the resolver granted this (singleton-calling) UE an UL grant — set with ONE
// fire-and-forget atomicOr by the UE's owner workgroup, consumed by the next pass's apply
constexpr unsigned PK_GRANT_BIT = 0x80000000u;
// ordered "special" events handed to the resolver
constexpr int EV_CALLER = 1, EV_RESETCAND = 2, EV_PASSIVE = 3, EV_RJOIN = 4;

struct alignas(16) Event {
    int idx;  // UE index
    int info; // type | bucket p << 8 | old bucket q << 16
    int le;   // #pre-members of bucket p with index <= idx
    int pad;
};

struct DevResult {
    int status, time_exit, nSuccess, collisionPreambles, totalPreambleTxop, activeCheck, continueFailed,
        finalSuccess, ptcSum, fcSum;
    unsigned long long draws, steps;
    long long sumTimer;
    unsigned long long dbg[4];
    unsigned long long stamps6[8]; // diagnostic build: cycles per phase (pass, publish, barrier, gather, resolve, grants)
    unsigned long long fstamps[24]; // diagnostic build: finer split (prach_cluster.hip FSTAMP)
    unsigned long long visits, events; // one workgroup per trial: 64-UE group visits of the pass, UEs through the event body (the kernel's OWN memory work)
    int hard_error;                    // a workgroup of the trial left with PRACH_ERR_INTERNAL (a per-subframe capacity): wins over a peer's PRACH_ERR_TIMEOUT in `status`
    int pad_;
};

struct TrialDev {
    int variant, uniform, nUE, nP, backoff, nGrantUL, maxRarWindow, maxMsg2, aT, rng_mode, maxTime, stop;
    unsigned seed_lo, seed_hi;
    unsigned long long stream_len;
    int4 *rec;
    int *ptc, *ftt, *stt, *fcnt; // cold per-UE fields: preambleTxCounter, firstTxTime, secondTxTime, failCount
    unsigned *nd;                // philox: per-UE draw index
    Event *evbuf, *evbuf2;       // event scratch (per-wave segments / compacted)
    int *sidx;                   // singleton-caller scratch
    const int *sched;            // arrival schedule (activeCheck per access slot)
    const int *stream;           // glibc mode: draw stream window
    prach_ue_log *logs;          // nullable
    int *timers;                 // per UE: final timer if succeeded, else INT_MIN
    DevResult *out;
    // cluster kernel (prach_cluster.hip) only
    int evw, mbstride;           // events per mailbox, mailbox stride (ints)
    int binshift;                // grant selection: UE index >> binshift < 1024
    int *mbox;                   // [2][G][mbstride] write-through mailboxes
    int2 *cand;                  // early-leaver candidate scratch, nUE + 64*G entries
    int dense_pass;              // 1: every group through the full per-UE body (diagnostic option); 0: compacted pass
    int pipeline;                // 1: clusters run phase A of the next subframe during the exchange of the current one
    // NOMA.c variant (prach_noma.hip) only: the host-built activation table
    const int *n_pre0, *n_sector;
    const double *n_gain, *n_lgain;
    const unsigned *n_nd0;
    float cell_radius;           // NOMA.c:56,168 (the UE drop of activeUE)
    int n_devact;                // 1: the table was built on the device (noma_activation_kernel): the resolver checks its gain comparisons against the error band
    int flags;                   // PRACH_FLAG_* (include/prach.h)
    int *sector;                 // PRACH_FLAG_SECTOR_GRANTS: per UE, the sector drawn by activateUEs (WithNOMA:393-410); else null
    // batch kernel (prach_batch.hip) only
    int4 *rec32;                 // [nUE][2] the 32-byte event record
    int4 *chunks;                // [nchunks][128] the pool of 2 KB chunks: the records of 64 UEs whose next event falls into one subframe
    int *ctab;                   // [calmask + 1][tcap] chunk table: the chunks of every future subframe's event list
    int *cpool;                  // [2][nchunks] shared pool of free chunk ids
    int nchunks, tcap;
    int *jcal;                   // [calmask + 1][calcap] join lists: the UEs whose contention window opens in a subframe
    int calcap, calmask;         // entries per join list; calendar slots - 1 (slot = subframe & calmask)
    int *qov;                    // [nUE] early-leaver candidates of a subframe beyond their LDS part
    int2 *evov;                  // [2 nUE] the resolver's event list of a subframe beyond its LDS part
    unsigned long long *diag;    // diagnostic build (PRACH_STAMPS) only: [CLUSTER_MAX_G][32] per-workgroup phase stamps of a cluster trial; else null
    // prach_run_trials_trace only (else null): [maxTime] one row per subframe, zeroed before the launch — x preambleCollision calls, y the calls with
    // check == 1, z what the subframe added to totalPreambleTxop, w what it added to collisionPreambles.  Written by ONE lane behind the barrier that closes
    // the subframe's calls (cluster_kernel: by the workgroup that writes DevResult; batch_kernel; trial_kernel), only where a call was made.
    // prach_run_trials_noma_trace (NOMA.c, else null): [access slots][6 sectors][2] — tx, used, singles, granted | pairs, pair_one, 0, 0 — written by lane 0 of
    // the sector's resolver wavefront of workgroup 0 (noma_kernel), only where somebody transmitted
    int4 *trace;
};

constexpr int WG_THREADS = 1024;
constexpr int NW = WG_THREADS / 64; // waves per workgroup
constexpr int EVCAP = 1024;         // events staged in LDS (more: resolved from global scratch)
constexpr int SCAP = 1024;          // singleton callers staged in LDS
constexpr int RCCAP = 256;          // reset-cycle re-join candidates per subframe

// host side, every kernel with dynamic LDS: raise the kernel's dynamic-LDS ceiling to `lds` and launch it; and the workgroups of the kernel
// (threads, that much dynamic LDS) the runtime admits per CU — at least 1, also when the query fails
template <class... KA, class... A>
inline hipError_t launch_with_lds(void (*fn)(KA...), int grid, int threads, size_t lds, hipStream_t stream, A... args) {
    const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, stream, args...);
    return hipGetLastError();
}
template <class... KA>
inline int kernel_blocks_per_cu(void (*fn)(KA...), int threads, size_t lds) {
    int nb = 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(fn), threads, lds) != hipSuccess || nb < 1) return 1;
    return nb;
}

size_t trial_kernel_lds_bytes(int nP);
hipError_t launch_trial_kernel(const TrialDev *params, int ntrials, int rng_mode, int maxP, hipStream_t stream);
size_t cluster_kernel_lds_bytes(int nP, bool glibc, int lslots);
// rec_mode: where / how a trial's hot records are kept (prach_cluster.hip): 0 global 16 B, 1 global 8 + 4 B (one workgroup per
// trial, the reference's rand() stream), 2 LDS-resident (clusters, Philox; lslots = owned UE slots per workgroup, the launch's maximum)
constexpr int CLUSTER_REC_G16 = 0, CLUSTER_REC_H8 = 1, CLUSTER_REC_L16 = 2;
constexpr int CLUSTER_EVW = 512;   // special-event granules per cluster mailbox and subframe
constexpr int CLUSTER_REC_LFAST = 3; // prach_lcluster.hip: the lean LDS-resident kernel (Philox clusters, nPreamble <= 64)
size_t lcluster_kernel_lds_bytes(int lslots, bool glibc = false, int groups = 0);
int lcluster_group_capacity(int groups);
int lcluster_max_groups_glibc();
int lcluster_max_preambles();
hipError_t launch_lcluster_kernel(const TrialDev *params, int ntrials, int G, int lslots, int xpack, bool glibc, int groups, hipStream_t stream);
constexpr int CLUSTER_LQCAP = 4096; // LDS-resident clusters: owned UE slots per workgroup at most (= the event queue)
constexpr size_t CLUSTER_LDS_LIMIT = 160 * 1024; // LDS per CU (MI355X_MICROARCH.md): one LDS-resident cluster workgroup per CU
hipError_t launch_cluster_kernel(const TrialDev *params, int ntrials, int G, int maxP, int rng_mode, int rec_mode, int lslots, int xpack, hipStream_t stream);
int cluster_kernel_blocks_per_cu(int maxP, int rng_mode, int rec_mode, int lslots); // occupancy query for the kernel and its dynamic LDS size
constexpr int CLUSTER_REC_BATCH = 4; // prach_batch.hip: one workgroup per trial, 4-byte pass words + 32-byte event records (Philox)
size_t batch_kernel_lds_bytes(int waves, bool glibc = false);
int batch_max_preambles();
int batch_max_rar_window();
int batch_max_subframes();
int batch_max_groups(bool glibc = false);
int batch_max_rar_window_two_per_cu();
int batch_chunk_bytes();
int batch_calendar_slots(int backoff, int accessTime, int maxRarWindow);
int batch_max_calendar_slots();
hipError_t launch_batch_kernel(const TrialDev *params, int ntrials, int waves, bool glibc, hipStream_t stream);
constexpr int STREAM_CHUNK = 31 * 2048; // rand() outputs generated per wavefront (prach_stream.hip)
hipError_t launch_glibc_stream(const unsigned *seeds, int *out, unsigned long long n, hipStream_t stream);
struct StreamJob { const unsigned *seeds; int *out; unsigned long long n; }; // one trial's window: a 31-word seed window per chunk, n values out
hipError_t launch_glibc_stream_jobs(const StreamJob *jobs, int njobs, unsigned long long max_n, hipStream_t stream); // (jobs: device memory)
extern "C" void prach_internal_glibc_seeds(uint32_t seed, uint64_t first, uint64_t nchunks, uint64_t chunk, uint32_t *out);
constexpr int CLUSTER_GLIBC_MAX_UE = 4096 * 64; // glibc mode on the cluster kernel: per-group draw counts live in LDS
constexpr int CLUSTER_MAX_G = 64;
size_t noma_kernel_lds_bytes(int nP);
hipError_t launch_noma_kernel(const TrialDev *params, int ntrials, int G, int maxP, int xpack, hipStream_t stream);
int noma_kernel_blocks_per_cu(int maxP);
// activeUE (NOMA.c:131-192) for every UE of every trial of a Philox launch, on the device.  flags[0]: number of UEs whose result may differ
// from the host libm's (a value within the error band of a rounding or comparison boundary); flags[2 + 2 q], flags[3 + 2 q]: trial, UE index
// of the q-th (q < cap).  The engine recomputes those with prach_noma_activation_range before the simulation kernel starts.
constexpr int NOMA_ACT_FLAG_CAP = 8192;
constexpr int NOMA_AMBIGUOUS = 77; // DevResult::hard_error: a gain comparison of the resolver fell inside the error band (the trial is rerun with the host-built table)
hipError_t launch_noma_activation(const TrialDev *params, int ntrials, int maxUE, unsigned *flags, hipStream_t stream);
// NOMA_C in the reference's own rand() stream (prach_noma_glibc.hip), both forms on the engine's arena and pinned mirror.  One launch:
//   [ TrialArgs[n] | control blocks | finishing blocks | StreamJob[n] | per trial: arrival table, stream seeds ]   staged: built in the mirror, ONE copy
//   [ per trial: UE records, stream window, list of live UEs, timers, ptc, log records where asked for ]
// The slot-by-slot form (`slots`, one trial) has no argument blocks, jobs and seeds — the host keeps the stream and uploads the window — and its UE records
// are part of the staged region: the host writes the arrivals' records there slot after slot.
struct NomaGlibcTrial { size_t sched, seeds, ue, stream, live, timers, ptc, logs, nsched, nchunks; unsigned long long len; }; // arena offsets (logs 0: none)
struct NomaGlibcLayout {
    std::vector<NomaGlibcTrial> t;
    bool slots = false;
    int max_ue = 0;
    size_t ue_bytes = 0, args = 0, ctl = 0, ctl_bytes = 0, live_state = 0, fin = 0, jobs = 0, staged_end = 0, end = 0; // ue_bytes: one UE record; ctl .. + ctl_bytes: what comes back after a launch
};
// what a trial's control block says after a launch, in either form.  status: PRACH_OK, PRACH_ERR_STREAM (window too small: once more with a larger one) or
// NOMA_GLIBC_AMBIGUOUS_RC (single-launch form: a value inside the device libm's error band — run that trial slot by slot); done (slot form): no slot is left
constexpr int NOMA_GLIBC_AMBIGUOUS_RC = -1077;
struct NomaGlibcEnd { unsigned long long pos, steps; int status, nSuccess, time_exit, activeCheck; long long delay; int nTxP, failed; bool done; };
NomaGlibcLayout noma_glibc_layout(const prach_cfg *cfgs, const int *idx, int n, const unsigned long long *lens, prach_ue_log *const *ue_logs, bool slots);
// fills the staged region of the mirror H for the arena A (every block zeroed first); nAccess[j]: prach_result.nAccessUE of trial j
void noma_glibc_stage(const NomaGlibcLayout &L, const prach_cfg *cfgs, const int *idx, const char *A, char *H, int32_t *nAccess);
hipError_t launch_noma_glibc_trials(const NomaGlibcLayout &L, const char *A, hipStream_t stream); // stream windows, noma_glibc_trial_kernel, the finishing kernel
// slot form, the access slot at subframe t: activates the arrivals [from, to) in the mirror with the reference's libm (hstream: the host copy of the window,
// *pos moves behind their draws) and fills the slot's control block; PRACH_OK or PRACH_ERR_STREAM
int noma_glibc_stage_slot(const NomaGlibcLayout &L, const prach_cfg &c, const int32_t *hstream, uint64_t *pos, int t, int from, int to, char *H);
hipError_t launch_noma_glibc_slot(const NomaGlibcLayout &L, const prach_cfg &c, const char *A, hipStream_t stream);
hipError_t launch_noma_glibc_finish(const NomaGlibcLayout &L, const char *A, hipStream_t stream);
NomaGlibcEnd noma_glibc_end(const NomaGlibcLayout &L, const prach_cfg &c, const char *H, int j);

// The reducer kernels below.  What they share is in prach_reduce_tile.h, ONE copy: the job lookup over `wg0`, the 64-bit agent-scope add and maximum, the
// wavefront folds, the slot range of a tile of UEs with its staging rule (TILE_SCHED_CAP), and the flush of a group's scalar row — the first *_SUMS words of
// a row are sums, the next *_MAXIMA maxima (stored + 1, so that 0 means none), both flushed only where non-zero; the counts stand next to *_SCALARS.
//
// prach_dist.hip: the distributions of a launch's accepted trials (prach_run_trials_dist).  One job per trial; a workgroup reduces one tile of
// DIST_TILE UEs of one trial in LDS and flushes its non-zero bins into the call's buffers with 64-bit device-scope atomics.
constexpr int DIST_TILE = 8192, DIST_THREADS = 256;
constexpr int DIST_SCALARS = 8, DIST_SUMS = 4, DIST_MAXIMA = 1; // per group: success, delay_overflow, delay_sum, ptc_sum | delay_max + 1 (0: no successful UE) | 3 spare
struct DistJob {
    const int *timers; // [nUE] the delay of a successful UE, INT_MIN otherwise
    const int *ptc;    // form 0: [nUE] preambleTxCounter; form 1: the 32-byte records of prach::batch_kernel (word 5 of a record, low half)
    int nUE, group, wg0, form; // wg0: the first workgroup of this job
};
hipError_t launch_dist_kernel(const DistJob *jobs, int njobs, int workgroups, int delay_bins, int delay_bin_ms, int scheme, unsigned long long *delay_hist,
                              unsigned long long *ptc_hist, unsigned long long *scalars, hipStream_t stream);

// prach_timeline.hip: the timelines of a launch's accepted trials (prach_run_trials_timeline).  One job per trial; a workgroup reduces one tile of
// TL_TILE consecutive UEs of one trial from the 64-byte log records the simulation kernel wrote on the device and from the trial's arrival schedule.
// scheme 1 privatises TL_WINDOW bins from the tile's first arrival bin on in LDS (four 32-bit counters per by-arrival bin, one per done bin) and
// flushes the non-zero ones; what falls outside, and everything under scheme 0, goes straight to the call's buffers with 64-bit agent-scope atomics.
constexpr int TL_TILE = 8192, TL_THREADS = 256, TL_WINDOW = 2048;
constexpr int TL_MAX_SOJOURN = 60000 + 6; // c(i) - a(i) at most: Uniform arrivals run 60 000 subframes, the completion is 6 behind the last Msg3
static_assert((unsigned long long)TL_TILE * TL_MAX_SOJOURN < (1ull << 32), "a 32-bit LDS counter holds the sojourn sum, and the timer sum, of a whole tile");
constexpr int TL_SCALARS = 8, TL_SUMS = 7, TL_MAXIMA = 1; // per group: arrived, success, restarted, arrival_overflow, done_overflow, sojourn_sum, timer_sum | done_max + 1 (0: no successful UE)
struct TimelineJob {
    const int4 *logs; // [nUE][4] prach_ue_log records
    const int *sched; // [nslots] activeCheck after the arrival update of every access slot
    int nUE, group, wg0, aT, nslots, pad; // wg0: the first workgroup of this job
};
struct TimelineOut { unsigned long long *arrivals, *success, *sojourn, *timer, *done, *scalars; }; // [ngroups][bins] each, [ngroups][TL_SCALARS]
hipError_t launch_timeline_kernel(const TimelineJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, TimelineOut out, hipStream_t stream);

// prach_sojourn.hip: the sojourn histograms by arrival row of a launch's accepted trials (prach_run_trials_sojourn).  The jobs are the timeline's
// (TimelineJob: log records and schedule of one trial), and so are tile and workgroup: one tile of TL_TILE consecutive UEs of one trial per workgroup.
// scheme 1 privatises the first R = min(rows from the tile's first arrival row on, SJ_WINDOW_WORDS / delay_bins) rows in LDS, one 32-bit counter per
// cell plus one arrived and one overflow counter per row, and flushes the non-zero ones; what falls outside, and everything under scheme 0, goes
// straight to the call's buffers with 64-bit agent-scope atomics.
constexpr int SJ_WINDOW_WORDS = 28672; // 112 KiB of cells, fourteen 500 ms rows of 2002 five-millisecond bins: measured against 8192 and 16384 words
static_assert((unsigned long long)TL_TILE < (1ull << 32), "a 32-bit LDS counter holds what one tile adds to a cell or a row: at most one per UE");
constexpr int SJ_SCALARS = 8, SJ_SUMS = 6, SJ_MAXIMA = 1; // per group: arrived, success, restarted, arrival_overflow, delay_overflow, sojourn_sum | sojourn_max + 1 (0: no successful UE) | 1 spare
struct SojournOut { unsigned long long *hist, *row_arrived, *row_overflow, *scalars; }; // [ngroups][rows][delay_bins], [ngroups][rows] twice, [ngroups][SJ_SCALARS]
hipError_t launch_sojourn_kernel(const TimelineJob *jobs, int njobs, int workgroups, int rows, int row_ms, int delay_bins, int delay_bin_ms, int scheme, SojournOut out,
                                 hipStream_t stream);

// prach_xtab.hip: the outcome cross-tabulation of a launch's accepted trials (prach_run_trials_xtab).  The jobs are the timeline's (TimelineJob: log records
// and schedule of one trial) with E = min(steps, maxTime) in `pad`, and so are tile and workgroup.  scheme 1 privatises a table of at most XT_WINDOW_WORDS
// cells in LDS, whole, as 32-bit counters and flushes the non-zero ones; a larger table, and everything under scheme 0, goes straight to the call's buffer
// with 64-bit agent-scope atomics.
constexpr int XT_WINDOW_WORDS = SJ_WINDOW_WORDS; // the sojourn kernel's measured window
static_assert((unsigned long long)TL_TILE < (1ull << 32), "a 32-bit LDS counter holds what one tile adds to a cell: at most one per UE");
constexpr int XT_SCALARS = 16, XT_SUMS = 7, XT_MAXIMA = 2; // per group: idle, served, unserved, selected, binned, row_sum, col_sum | row_max + 1, col_max + 1 (0: nothing binned) | 7 spare
struct XtabAxes { int who, row_field, row_width, row_bins, col_field, col_width, col_bins; };
struct XtabOut { unsigned long long *cells, *scalars; }; // [ngroups][row_bins + 1][col_bins + 1], [ngroups][XT_SCALARS]
hipError_t launch_xtab_kernel(const TimelineJob *jobs, int njobs, int workgroups, XtabAxes ax, int scheme, XtabOut out, hipStream_t stream);

// prach_summary.hip: one summary row per accepted trial of a launch (prach_run_trials_summary).  The jobs are the timeline's (TimelineJob: log records and
// schedule of one trial; group = the row), ONE workgroup per trial.  A row is SM_WORDS 64-bit words, written with plain stores: arrived, success, restarted,
// 3 range-error counts [sojourn, timer, preambleTxCounter], 3 sums, 3 maxima (-1: no successful UE), then [3][PRACH_SUMMARY_MAX_Q] levels (-1: not found or unused).
constexpr int SM_WORDS = 12 + 3 * PRACH_SUMMARY_MAX_Q;
constexpr int SM_MAX_VALUE = 65535; // the largest value the two-level selection ranks (prach_summary_max_value)
struct SummaryLevels { int nq; int permille[PRACH_SUMMARY_MAX_Q]; };
// threads: 512 or 1024; sched_cap: schedule entries staged in LDS (the longest schedule of the jobs, cut to summary_sched_cap())
int summary_sched_cap();
hipError_t launch_summary_kernel(const TimelineJob *jobs, int njobs, SummaryLevels levels, int threads, int sched_cap, unsigned long long *rows, hipStream_t stream);

// prach_pick.hip: the pick of every accepted trial of a launch (prach_run_trials_pick).  The jobs are the timeline's with E = min(steps, maxTime) in `pad`
// (group = the trial's row block), ONE workgroup per trial.  Per trial the kernel stores up to spec.k rows of PK_ROW_WORDS 64-bit words (prach_pick_row: the
// 64-byte log record, a(i), the key, two zero words) IN UE-INDEX ORDER — the engine sorts them into the defined order — and PK_SCALARS 64-bit scalars:
// selected, matched, stored, undefined, range_errors, threshold (signed, -1: nothing stored), ties_left_out, 0.  Plain stores; rows behind `stored` are not
// written.
constexpr int PK_ROW_WORDS = 10, PK_SCALARS = 8;
static_assert(8 * PK_ROW_WORDS == sizeof(prach_pick_row) && sizeof(prach_pick_row) % 16 == 0 && alignof(prach_pick_row) == 8, "a row is five 16-byte stores");
extern "C" int prach_internal_pick_spec_ok(const prach_pick_spec *spec); // prach_host.c
// threads: 512 or 1024; sched_cap: schedule entries staged in LDS (the longest schedule of the jobs, cut to pick_sched_cap()); spec: a valid one
int pick_sched_cap();
hipError_t launch_pick_kernel(const TimelineJob *jobs, int njobs, prach_pick_spec spec, int threads, int sched_cap, unsigned long long *rows, unsigned long long *scalars,
                              hipStream_t stream);

// prach_columns.hip: the per-UE columns of a launch's accepted trials (prach_run_trials_columns, prach_run_trials_columns_device).  The jobs are the timeline's
// with E = min(steps, maxTime) in `pad` (group = the trial), and so are tile and workgroup.  Column c of UE i of trial k is the 32-bit word
// data[c * stride + offset[k] + i]: `data` is the call's own buffer or device memory of the caller's, `offset` the call's table of first rows, one per trial.
// Plain 4-byte stores; what no job names is not written.  Per trial CL_SCALARS 64-bit scalars, added with agent-scope atomics: idle, served, unserved | 1 spare.
constexpr int CL_SCALARS = 4, CL_SUMS = 3;
struct ColumnsOut { int *data; unsigned long long stride; const unsigned long long *offset; unsigned long long *scalars; }; // stride in words; [ntrials], [ntrials][CL_SCALARS]
extern "C" int prach_internal_columns_spec_ok(const prach_columns_spec *spec); // prach_host.c
hipError_t launch_columns_kernel(const TimelineJob *jobs, int njobs, int workgroups, const prach_columns_spec &spec, ColumnsOut out, hipStream_t stream); // spec: a valid one

// prach_noma_census.hip: the census and the columns of a launch's accepted NOMA.c trials over THE NOMA MENU of include/prach.h (prach_run_trials_noma_census,
// prach_run_trials_noma_columns, _device).  Jobs, tile, workgroup, table paths and column layout are those of prach_xtab.hip and prach_columns.hip above; NOMA
// has four classes, so a group's scalar row and a trial's count one more.
constexpr int NC_SCALARS = XT_SCALARS, NC_SUMS = 8, NC_MAXIMA = XT_MAXIMA; // per group: idle, served, dropped, pending, selected, binned, row_sum, col_sum | row_max + 1, col_max + 1 (0: nothing binned) | 6 spare
constexpr int NCL_SCALARS = CL_SCALARS, NCL_SUMS = 4;                      // per trial: idle, served, dropped, pending
static_assert(NC_SCALARS == XT_SCALARS && NC_MAXIMA == XT_MAXIMA && NCL_SCALARS == CL_SCALARS, "one row size per kind for both menus: the kernels' bodies are shared (prach_menu_body.h)");
extern "C" int prach_internal_noma_census_spec_ok(const prach_xtab_spec *spec);     // prach_host.c
extern "C" int prach_internal_noma_columns_spec_ok(const prach_columns_spec *spec); // prach_host.c
hipError_t launch_noma_census_kernel(const TimelineJob *jobs, int njobs, int workgroups, XtabAxes ax, int scheme, XtabOut out, hipStream_t stream); // ax: a valid spec's
int noma_census_copy_words(); // LDS words that the per-wavefront copies of a census table take at most
hipError_t launch_noma_columns_kernel(const TimelineJob *jobs, int njobs, int workgroups, const prach_columns_spec &spec, ColumnsOut out, hipStream_t stream); // spec: a valid one

// prach_noma_select.hip: the summary row and the pick of every accepted NOMA.c trial of a launch over THE NOMA MENU (prach_run_trials_noma_summary, _noma_pick).
// The jobs are the timeline's with E = min(steps, maxTime) in `pad` (group = the trial), ONE workgroup per trial, plain stores.
// SUMMARY: a row is NSM_WORDS 64-bit words: idle, served, dropped, pending, selected, restarted, 4 range-error counts, 4 counts n[x], 4 sums, 4 maxima (-1:
// n[x] == 0), then [4][PRACH_SUMMARY_MAX_Q] levels (-1: not found or unused).  PICK: rows (PK_ROW_WORDS) and scalars (PK_SCALARS) are those of prach_pick.hip
// above; `who`, the clause fields and the key field of the spec are PRACH_NOMA_*.
constexpr int NSM_WORDS = 22 + PRACH_NOMA_SUMMARY_MAX_FIELDS * PRACH_SUMMARY_MAX_Q;
extern "C" int prach_internal_noma_summary_spec_ok(const prach_noma_summary_spec *spec); // prach_host.c
extern "C" int prach_internal_noma_pick_spec_ok(const prach_pick_spec *spec);            // prach_host.c
// threads: 512 or 1024; sched_cap: schedule entries staged in LDS (the longest schedule of the jobs, cut to noma_select_sched_cap()); spec: a valid one
int noma_select_sched_cap();
hipError_t launch_noma_summary_kernel(const TimelineJob *jobs, int njobs, prach_noma_summary_spec spec, int threads, int sched_cap, unsigned long long *rows, hipStream_t stream);
hipError_t launch_noma_pick_kernel(const TimelineJob *jobs, int njobs, prach_pick_spec spec, int threads, int sched_cap, unsigned long long *rows, unsigned long long *scalars,
                                   hipStream_t stream);

// prach_trace.hip: the per-subframe preamble trace of a launch's accepted trials (prach_run_trials_trace).  One job per trial: the rows the simulation kernel
// wrote through TrialDev::trace, for the subframes [0, steps).  A workgroup reduces one tile of TR_TILE consecutive subframes of one trial, 16 bytes per lane
// and load.  A tile covers at most TR_TILE consecutive bins (bin = t / bin_ms): scheme 1 adds them up in an LDS window of 64-bit counters anchored at the
// tile's first bin and flushes the non-zero ones, scheme 0 sends every contribution straight to the call's buffers; both with 64-bit agent-scope atomics.
constexpr int TR_TILE = 2048, TR_THREADS = 256;
constexpr int TR_SCALARS = 8, TR_SUMS = 6, TR_MAXIMA = 1; // per group: subframes, calls, singles, txop, collisions, overflow_calls | calls_max + 1 (0: no subframe) | 1 spare
struct TraceJob {
    const int4 *rows; // [steps] calls, singles, txop, collisions of every subframe
    int steps, group, wg0, pad; // wg0: the first workgroup of this job
};
struct TraceOut { unsigned long long *calls, *singles, *txop, *collisions, *scalars; }; // [ngroups][bins] each, [ngroups][TR_SCALARS]
hipError_t launch_trace_kernel(const TraceJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, TraceOut out, hipStream_t stream);

// prach_noma_trace.hip: NOMA.c's channel trace of a launch's accepted trials (prach_run_trials_noma_trace).  One job per trial: the rows prach::noma_kernel
// wrote through TrialDev::trace, two 16-byte words per (access slot, sector) — tx, used, singles, granted | pairs, pair_one, 0, 0 — row r being slot r / 6,
// sector r % 6, for the slots whose subframe lies in [0, steps).  A workgroup reduces one tile of NT_TILE consecutive rows (NT_TILE / 6 whole slots) of one
// trial.  Slot s falls into bin s * aT / bin_ms: scheme 1 adds a tile up in an LDS window of 64-bit counters, NT_WINDOW bins from the tile's first on, and
// flushes the non-zero ones; what falls behind the window (bin_ms < aT only), and everything under scheme 0, goes straight to the call's buffers; both with
// 64-bit agent-scope atomics.
constexpr int NT_TILE = 768, NT_THREADS = 256, NT_WINDOW = NT_TILE / 6;
static_assert(NT_TILE % 6 == 0 && NT_TILE % NT_THREADS == 0, "a tile is whole slots, and whole passes of the workgroup");
constexpr int NT_SCALARS = 12, NT_SUMS = 8, NT_MAXIMA = 1; // per group: slots, tx, used, singles, granted, pairs, pair_one, overflow_tx | tx_max + 1 (0: no row) | 3 spare
struct NomaTraceJob {
    const int4 *rows; // [nrows][2]
    int nrows, group, wg0, aT; // wg0: the first workgroup of this job
};
struct NomaTraceOut { unsigned long long *series[6], *scalars; }; // [ngroups][6 sectors][bins] each, [ngroups][NT_SCALARS]
hipError_t launch_noma_trace_kernel(const NomaTraceJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, NomaTraceOut out, hipStream_t stream);

// prach_noma_timeline.hip: NOMA.c's timelines per sector of a launch's accepted trials (prach_run_trials_noma_timeline).  The jobs are the timeline's with
// E = min(steps, maxTime) in `pad`, and so are tile and workgroup: one tile of TL_TILE consecutive UEs of one trial.  scheme 1 adds a tile up in an LDS window
// of 32-bit counters, `window` bins x 6 sectors x 6 series from the tile's first arrival bin on, and flushes the non-zero ones; what falls outside — a later
// arrival bin, a completion bin, a sojourn or timer above NTL_MAX_SOJOURN — and everything under scheme 0 goes straight to the call's buffers; both with 64-bit
// agent-scope atomics.  `window` is a launch argument (the LDS is dynamic): 1 .. NTL_WINDOW_MAX, NTL_WINDOW where nobody asks (profiles/noma_timeline_kernel.md).
constexpr int NTL_WINDOW = 256, NTL_WINDOW_MAX = 1024;
constexpr int NTL_MAX_SOJOURN = 10000 + 6; // c(i) - a(i) of a NOMA.c trial at most: 10 000 subframes, the completion is 6 behind the success (prach_noma_menu.h: THE BOUNDS)
static_assert((unsigned long long)TL_TILE * NTL_MAX_SOJOURN < (1ull << 32), "a 32-bit LDS counter holds the sojourn sum, and the timer sum, of a whole tile");
static_assert(4 * (2048 + 36 * NTL_WINDOW_MAX) + 8 * 12 <= 160 * 1024, "the largest window, the staged schedule range and the scalars fit the 160 KiB of LDS of a gfx950 CU");
constexpr int NTL_SCALARS = 12, NTL_SUMS = 10, NTL_MAXIMA = 1; // per group: idle, served, dropped, pending, undefined, restarted, arrival_overflow, done_overflow, sojourn_sum, timer_sum | done_max + 1 (0: no served UE) | 1 spare
struct NomaTimelineOut { unsigned long long *series[6], *scalars; }; // [ngroups][6 sectors][bins] each: arrivals, served, dropped, sojourn_sum, timer_sum, done; [ngroups][NTL_SCALARS]
hipError_t launch_noma_timeline_kernel(const TimelineJob *jobs, int njobs, int workgroups, int bins, int bin_ms, int scheme, int window, NomaTimelineOut out, hipStream_t stream);

// prach_noma_gain.hip: NOMA.c's near-far profile of a launch's accepted trials (prach_run_trials_noma_gain).  A job is the timeline's with E in `pad`, plus the
// trial's ln(gain) column of the activation table and its 4-byte-per-UE LEVEL column; tile and workgroup are the timeline's.  Two kernels:
//   the level pre-pass   level[i] = floor(1000 x lgain[i]) for every UE of every job; a UE whose product lies within NG_LEVEL_BAND of an integer, outside the
//                        range the band is derived for, or that has no level is EDGE: appended as (job, UE) to a list of NG_EDGE_CAP entries behind two
//                        header words (the count — which goes on counting past the capacity — and a spare), for the host to resolve;
//   the reducer          scheme 1 keeps all 6 series x 6 sectors x bins 32-bit counters of a tile in LDS when bins <= NG_LDS_MAX_BINS and flushes the non-zero
//                        ones; otherwise, and under scheme 0, everything goes straight to the call's buffers.  Both with 64-bit agent-scope atomics.
// THE BAND.  With a device-built table (n_devact) the gain of an unflagged UE is within ACT_GAIN_ULP_ASSERTED ulps of the host libm's (prach_noma_act.h), so
// ln g is off by at most that many ulps of 1.0 (d ln g = dg / g) plus the ulps of the two logarithms themselves (NG_LOG_ULPS for the device's, one for the
// host's), each an ulp of a value below 32 (a trial's |ln g| is below 16.2): 2^-48.  Times 1000, plus one ulp of the product (two roundings of half an ulp of a
// value below 2^15: 2^-37).  The band is a hundred times that.
constexpr int NG_EDGE_CAP = 4096;
constexpr double NG_LEVEL_RANGE = 32768.0; // |1000 ln g| below this: what the band is derived for (a product outside is EDGE)
constexpr int NG_LOG_ULPS = 2;
constexpr double NG_LEVEL_BAND = 1e-8;
constexpr double NG_LEVEL_ERROR = 1000.0 * (32 /* ACT_GAIN_ULP_ASSERTED */ * 0x1p-52 + (NG_LOG_ULPS + 1) * 0x1p-48) + 0x1p-37;
static_assert(NG_LEVEL_BAND >= 100.0 * NG_LEVEL_ERROR, "the level band covers the error of 1000 ln g of a device-built table a hundred times over");
static_assert(NG_LEVEL_BAND < 1e-6, "... and stays narrow: about 2 x band of the UEs go to the host");
constexpr int NG_LDS_MAX_BINS = 511;
static_assert(4 * (2048 + 36 * NG_LDS_MAX_BINS) + 8 * 16 <= 80 * 1024, "the counters, the staged schedule range and the scalars take at most half the 160 KiB of LDS of a gfx950 CU: two workgroups per CU");
constexpr int NG_MAX_ADDEND = NTL_MAX_SOJOURN; // a sojourn, lost time or preamble count up to this goes into a tile's 32-bit LDS counter; a larger one straight out
constexpr int NG_SCALARS = 16, NG_SUMS = 12, NG_MAXIMA = 2; // per group: idle, served, dropped, pending, undefined, below, above, restarted, sojourn_sum, lost_sum, ptc_sum, defined | level_max + 2^31, -level_min + 2^31 (0: no defined UE) | 2 spare
struct NomaGainJob : TimelineJob {
    const double *lgain; // [nUE] the activation table's ln(gain)
    int *level;          // [nUE] the level column
};
struct NomaGainOut { unsigned long long *series[6], *scalars; }; // [ngroups][6 sectors][bins] each: arrived, served, dropped, sojourn_sum, lost_sum, ptc_sum; [ngroups][NG_SCALARS]
hipError_t launch_noma_gain_levels(const NomaGainJob *jobs, int njobs, int workgroups, unsigned *edges, int edge_cap, hipStream_t stream); // edges: [2 + 2 x edge_cap], zeroed
hipError_t launch_noma_gain_kernel(const NomaGainJob *jobs, int njobs, int workgroups, int bins, int width, int lo, int scheme, NomaGainOut out, hipStream_t stream);

} // namespace prach
