/* include/prach.h — C ABI of libprach_hip.so, the MI355X-native replacement for the reference's
 * per-subframe PRACH random-access simulation loop.
 *
 * The reference (yaki-toki/5G-NR-RandomAccess) has no library/FFI seam: each program inlines the
 * trial body in main() between calloc and free (RandomAccessSimulatorBeta.c:75-210,
 * RandomAccessWithNOMA.c:226-368, NOMA.c:650-714).  This header is the seam a maintainer would cut
 * there: ONE call per batch of (seed, nUE) trials replaces
 *     initialUE            Beta.c:220   WithNOMA:374
 *     activation loop      Beta.c:121-147 / activateUEs WithNOMA:383
 *     selectPreamble       Beta.c:229   WithNOMA:475
 *     preambleCollision    Beta.c:315   WithNOMA:607
 *     requestResourceAllocation Beta.c:371 WithNOMA:667
 *     timerIncrease        Beta.c:413   WithNOMA:712
 *     successUEs           Beta.c:421   WithNOMA:720
 *     end-of-trial sums    Beta.c:185-197 WithNOMA:337-351
 * and the writers reproduce saveSimulationLog / saveResult (Beta.c:432-514, WithNOMA:731-825).
 * Plain C types only; no torch / HIP types cross this boundary.  INTEGRATION.md shows the stub a
 * maintainer adds on the reference side.
 */
#ifndef PRACH_H
#define PRACH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* which program's loop is reproduced (they differ: SURVEY.md §7.3) */
#define PRACH_VARIANT_BETA_C      0 /* RandomAccessSimulatorBeta.c */
#define PRACH_VARIANT_WITHNOMA_C  1 /* RandomAccessWithNOMA.c      */
#define PRACH_VARIANT_NOMA_C      2 /* NOMA.c (sector power-level grouping) */

/* prach_cfg.flags: variants the reference carries as commented-out code (never executed by the programs as committed) */
#define PRACH_FLAG_SECTOR_GRANTS   1 /* WITHNOMA_C: one UL-grant budget per 60-degree sector (sectorGrants[6], RandomAccessWithNOMA.c:260,
                                        271-273; the call of :312 and the grantCheck[sector] test of :626-637 un-commented); the sector
                                        comes from activateUEs' first draw (WithNOMA:393-410).  Runs on prach::batch_kernel (one workgroup
                                        per trial) in both RNG modes */
#define PRACH_FLAG_NOMA_NONSECTOR  2 /* NOMA_C: the cell-wide grouping preambleCollisionDetection (NOMA.c:325-447, call of :688
                                        un-commented) instead of preambleSectorCollisionDetection: one nGrantUL budget per access slot */

#define PRACH_RNG_GLIBC  0 /* the reference's own draw stream: srand(seed)/rand(), bit-exact vs the reference */
#define PRACH_RNG_PHILOX 1 /* Philox4x32-10, counter = (ue, draw#, nUE, variant), key = seed */

/* status codes (0 = ok).  The reference checks nothing and returns void everywhere; its only
 * error behaviour is the CLI's message + exit(-1) (WithNOMA:94-204), reproduced by prach_cli. */
#define PRACH_OK                 0
#define PRACH_ERR_ARG           -1 /* NULL pointer / non-positive nUE, nPreamble, backoff, accessTime ... */
#define PRACH_ERR_UNSUPPORTED   -2 /* nPreamble > 254, maxRarWindow > 255, maxMsg2TxCount > 255 */
#define PRACH_ERR_DEVICE        -3 /* HIP runtime error, no gfx950 device */
#define PRACH_ERR_STREAM        -4 /* glibc draw stream exhausted (engine retries internally) */
#define PRACH_ERR_INTERNAL      -5 /* device-side consistency check failed */
#define PRACH_ERR_IO            -6
#define PRACH_ERR_TIMEOUT       -7 /* a workgroup of a trial's cluster waited too long for a peer workgroup (the cluster was not
                                      wholly resident, e.g. another process holds CUs): the engine reruns such a trial on a
                                      kernel that waits for nobody and counts it in prach_timing; callers never see it */

typedef struct prach_cfg {
    int32_t variant;        /* PRACH_VARIANT_* */
    int32_t uniform;        /* 1: Uniform arrivals over 60 000 ms (Beta.c:92); 0: Beta(3,4) over 10 000 ms (Beta.c:103) */
    int32_t nUE;            /* Beta.c:75 */
    int32_t nPreamble;      /* Beta.c:47 */
    int32_t backoff;        /* backoffIndicator, Beta.c:48 */
    int32_t nGrantUL;       /* Beta.c:49; effective grants per 5 ms = value-1 (Beta.c:336-338) */
    int32_t maxRarWindow;   /* Beta.c:52 */
    int32_t maxMsg2TxCount; /* Beta.c:53 */
    int32_t accessTime;     /* Beta.c:54 */
    int32_t rng_mode;       /* PRACH_RNG_* */
    uint64_t seed;          /* srand(seed), Beta.c:69 */
    uint64_t stream_offset; /* glibc mode: rand() calls already consumed from this seed's stream
                               (the reference seeds once per seed and lets the stream run on across
                               the nUE sweep: Beta.c:66-71) */
    int32_t max_steps;      /* 0 = run to maxTime; >0 = stop after that many subframes */
    int32_t flags;          /* PRACH_FLAG_*: code paths the reference's author left commented out */
    float cellRadius, hBS, hUT; /* parsed by the CLI, never read by the simulation (WithNOMA:80-82);
                                   NOMA_C: cellRadius scales the UE drop (NOMA.c:56,168) */
} prach_cfg;

typedef struct prach_result {
    int32_t status;            /* PRACH_OK or error for this trial */
    int32_t time_exit;         /* `time` after the loop: printed "Total simulation time" (Beta.c:441) */
    int32_t maxTime;
    int32_t nSuccessUE;        /* Beta.c:178 */
    int32_t failedUEs;         /* Beta.c:185 */
    int32_t preambleTxCount;   /* Beta.c:194 */
    int32_t failCounts;        /* WithNOMA:348 */
    int32_t collisionPreambles, totalPreambleTxop; /* globals Beta.c:41-42 */
    int32_t activeCheck;       /* Beta.c:200 */
    int32_t nAccessUE;         /* Beta.c:95 */
    int32_t continueFaliedUEs, finalSuccessUEs; /* WithNOMA:84-85 */
    float totalDelay;          /* float running sum in index order, Beta.c:193 */
    int64_t sumTimer;          /* the same sum in exact integer arithmetic */
    uint64_t draws;            /* rand() calls consumed (glibc: add to stream_offset for the next trial) */
    uint64_t steps;            /* subframes executed; UE-subframe updates = nUE * steps */
} prach_result;

/* the 15 fields saveResult logs per UE (Beta.c:501-508) + failCount (WithNOMA:33) */
typedef struct prach_ue_log {
    int32_t idx, timer, active, txTime, firstTxTime, secondTxTime, nowBackoff, preamble, preambleChange,
        rarWindow, maxRarCounter, preambleTxCounter, msg2Flag, connectionRequest, msg4Flag, failCount;
} prach_ue_log;

typedef struct prach_timing {
    double kernel_ms;     /* HIP-event time of the simulation kernel launch(es) of the last call, on the engine's stream */
    double upload_ms;     /* host->device staging (schedules, parameters, glibc stream seeds; NOMA_C: the activation tables) */
    double total_ms;      /* wall time of the whole call */
    int32_t launches;     /* kernel launches in the last call */
    int32_t workgroups;   /* workgroups of the last launch */
    uint64_t updates;     /* sum over trials of nUE * steps */
    int32_t cluster_size;    /* workgroups per trial of the last launch (0: the one-workgroup fallback kernel) */
    int32_t resident_limit;  /* workgroups of a cluster launch that can be resident at once: one per CU (every cluster layout takes
                                more than half a CU's LDS; the runtime's occupancy query for the smallest one is the upper bound);
                                a cluster launch never exceeds it (its workgroups wait for each other) */
    int32_t fallback_trials; /* trials of the last call that a cluster launch could not finish and that were rerun (exactly) on
                                a kernel that waits for nobody: a per-subframe capacity exceeded, or a peer wait timed out.  Philox
                                trials go to prach::batch_kernel first (one workgroup per trial, event queue without a capacity);
                                trial_kernel_reruns (below) counts the ones that ended on the slow index-ordered trial_kernel */
    int32_t spin_timeouts;   /* ... of which: peer waits that timed out (PRACH_ERR_TIMEOUT) */
    int32_t rec_mode;        /* which kernel / record form the last cluster launch used: 0 prach::cluster_kernel, 16-byte records in global
                                memory; 1 the same with 8 + 4 byte records (one workgroup per trial: the glibc modes); 2 the same with
                                records resident in LDS (clusters, Philox); 3 prach::lcluster_kernel (the lean LDS-resident cluster
                                kernel: single Philox trials, the bench's N = 1 workload); 4 prach::batch_kernel (one workgroup per
                                trial, 4-byte pass words + 32-byte event records: the batched sweeps, Philox) */
    int32_t xcd_packed;   /* 1: the last cluster launch was XCD-packed (each cluster on the CUs of one XCD; prach_engine_set "xcd_pack") */
    uint64_t group_visits;   /* one workgroup per trial: 64-UE group visits of the pass, summed over the call */
    uint64_t event_ues;      /* ... and UEs that went through the full event body: the kernel's OWN memory work, for a roofline built from
                                the bytes it really moves (batch_kernel: a visit reads one 4-byte pass word per lane, an event reads and
                                writes one 32-byte record and one pass word) */
    int32_t trial_kernel_reruns; /* of fallback_trials: trials that were (also) rerun on the one-workgroup, index-ordered trial_kernel */
    int32_t noma_host_ues;       /* NOMA_C, Philox: UEs of the device-built activeUE table that the host recomputed with its libm (a value inside the
                                    device math library's error band of a rounding / comparison boundary: ~1e-6 of the UEs) */
    int32_t noma_gain_host_ues;  /* prach_run_trials_noma_gain: UEs whose gain level the host resolved in the last call (1000 ln g within the error band of an
                                    integer, or no level: ~2e-8 of the UEs; every UE of a launch whose list of such UEs overflowed); 0 in every other call */
    int32_t noma_gain_pad;       /* 0 */
    double noma_gain_ms;         /* HIP-event time of the gain-level pre-pass and the NOMA gain kernel launches (prach_run_trials_noma_gain) of the last call, the
                                    host's work on the listed UEs between the two included; 0 in every other call (such a call leaves every other *_ms of a
                                    reduction 0) */
    double noma_timeline_ms;     /* HIP-event time of the NOMA timeline kernel launches (prach_run_trials_noma_timeline) of the last call; 0 in every other call (such
                                    a call leaves every other *_ms of a reduction 0) */
    double noma_trace_ms;        /* HIP-event time of the NOMA trace kernel launches (prach_run_trials_noma_trace) of the last call; 0 in every other call (such a
                                    call leaves every other *_ms of a reduction 0) */
    double noma_summary_ms;      /* HIP-event time of the NOMA summary kernel launches (prach_run_trials_noma_summary) of the last call; 0 in every other call (such a
                                    call leaves every other *_ms of a reduction 0) */
    double noma_pick_ms;         /* HIP-event time of the NOMA pick kernel launches (prach_run_trials_noma_pick) of the last call; 0 in every other call (such a call
                                    leaves every other *_ms of a reduction 0) */
    double noma_census_ms;       /* HIP-event time of the NOMA census kernel launches (prach_run_trials_noma_census) of the last call; 0 in every other call (a
                                    census call leaves every other *_ms of a reduction 0) */
    double noma_columns_ms;      /* HIP-event time of the NOMA columns kernel launches (prach_run_trials_noma_columns, prach_run_trials_noma_columns_device) of the
                                    last call; 0 in every other call (such a call leaves every other *_ms of a reduction 0) */
    double columns_ms;           /* HIP-event time of the columns kernel launches (prach_run_trials_columns, prach_run_trials_columns_device) of the last call; 0 in
                                    every other call (a columns call leaves every other *_ms of a reduction 0) */
    double pick_ms;              /* HIP-event time of the pick kernel launches (prach_run_trials_pick) of the last call; 0 in every other call (a pick call
                                    leaves every other *_ms of a reduction 0) */
    double xtab_ms;              /* HIP-event time of the cross-tabulation kernel launches (prach_run_trials_xtab) of the last call; 0 in every other call (an
                                    xtab call leaves every other *_ms of a reduction 0) */
    double trace_ms;             /* HIP-event time of the trace kernel launches (prach_run_trials_trace) of the last call; 0 in every other call (a trace call leaves
                                    summary_ms, dist_ms, timeline_ms and sojourn_ms 0) */
    double summary_ms;           /* HIP-event time of the summary kernel launches (prach_run_trials_summary) of the last call; 0 in every other call (a summary call
                                    leaves dist_ms, timeline_ms and sojourn_ms 0) */
    double dist_ms;              /* HIP-event time of the distribution kernel launches (prach_run_trials_dist) of the last call; 0 without a spec */
    double timeline_ms;          /* HIP-event time of the timeline kernel launches (prach_run_trials_timeline) of the last call; 0 in every other call */
    double sojourn_ms;           /* HIP-event time of the sojourn kernel launches (prach_run_trials_sojourn) of the last call; 0 in every other call (a sojourn
                                    call leaves dist_ms and timeline_ms 0) */
} prach_timing;

typedef struct prach_engine prach_engine;

/* Engine lifetime: owns the HIP stream and every device buffer (nothing is allocated per subframe,
 * unlike preambleCollision's malloc per call, Beta.c:319).  device = HIP ordinal. */
int prach_engine_create(int device, prach_engine **out);
void prach_engine_destroy(prach_engine *);

/* Run n independent trials concurrently on the device (one workgroup cluster per trial).
 * ue_logs may be NULL; otherwise ue_logs[k] is NULL or a caller-owned array of cfgs[k].nUE entries. */
int prach_run_trials(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results,
                     prach_ue_log *const *ue_logs);
int prach_last_timing(const prach_engine *, prach_timing *out);

/* Distributions per trial group, built on the device: the histogram of the access delay (`timer`) and of the number of preamble
 * transmissions (`preambleTxCounter`) of the successful UEs (msg4Flag == 1; NOMA_C: RA == 1 and nTxPreamble) — the CDFs TR 37.868 and the
 * papers present next to the scalar results.  prach::dist_kernel (csrc/prach_dist.hip) reduces the per-UE state a simulation kernel leaves on
 * the device, so no per-UE log crosses the bus.  Integers only: merging is order-free and exact. */
#define PRACH_DIST_PTC_BINS        256     /* bin min(preambleTxCounter, 255) */
#define PRACH_DIST_MAX_DELAY_BINS  16384

typedef struct prach_dist_spec {
    int32_t delay_bins;    /* 1 .. PRACH_DIST_MAX_DELAY_BINS */
    int32_t delay_bin_ms;  /* >= 1; bin b counts successful UEs with b*w <= timer < (b+1)*w */
    int32_t ngroups;       /* number of output distributions */
    int32_t reserved;      /* 0 */
} prach_dist_spec;

typedef struct prach_dist {          /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                    /* sum of their nUE */
    uint64_t success;                /* UEs counted in the histograms (msg4Flag == 1) */
    uint64_t delay_overflow;         /* successful UEs with timer >= delay_bins * delay_bin_ms (in no delay bin) */
    uint64_t delay_sum, ptc_sum;     /* sum of timer / of preambleTxCounter over the successful UEs, unbinned */
    int64_t  delay_max;              /* -1 if success == 0 */
} prach_dist;

/* prach_run_trials plus the distributions: trial k is added to group group[k] (in [0, ngroups); group == NULL: trial k is group k and ngroups
 * must equal n).  delay_hist[ngroups * delay_bins], ptc_hist[ngroups * PRACH_DIST_PTC_BINS] and dist[ngroups] are caller-owned and OVERWRITTEN.
 * A trial whose final status is not PRACH_OK contributes nothing; a trial the engine reruns contributes once, from the launch whose result is kept.
 * PRACH_ERR_ARG: a NULL output, a bin count or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED: ngroups * (delay_bins + 256) > 2^27 words (1 GiB of device buffer). */
int prach_run_trials_dist(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results,
                          prach_ue_log *const *ue_logs, const prach_dist_spec *spec, const int32_t *group,
                          prach_dist *dist, uint64_t *delay_hist, uint64_t *ptc_hist);

/* Timeline per trial group, built on the device: what arrived, was served and completed in each stretch of the simulation.  Everything is derived from
 * fields every simulation kernel already logs, the UE index and the arrival schedule (no new simulation semantics).  For UE i of a trial with config cfg:
 *   a(i)  = accessTime x the first slot s with sched[s] > i, sched = prach_arrival_schedule(cfg) (UEs are activated in index order, Beta.c:121-147;
 *           a UE no slot activates has a(i) = accessTime x the number of slots, which is not below maxTime)
 *   UE i ARRIVED iff its logged active != -1
 *   a successful UE (msg4Flag == 1): txTime is the subframe of its successful Msg3, c(i) = txTime + 6 its completion, c(i) - a(i) its SOJOURN, and
 *           txTime + 6 - timer the start of its last attempt cycle; it RESTARTED iff that start differs from a(i)
 * The reference zeroes `timer` whenever a UE starts over (after maxMsg2TxCount retransmissions, Beta.c:250-281; after a Msg3 timeout, Beta.c:384-410): its
 * "access delay" is the length of the LAST cycle.  The sojourn is the time since the UE arrived; both sums are reported.
 * Bin b covers [b * bin_ms, (b + 1) * bin_ms).  Five series of `bins` entries per group:
 *   arrivals[b]     arrived UEs with a(i) in bin b
 *   success[b]      successful UEs with a(i) in bin b
 *   sojourn_sum[b]  sum of c(i) - a(i) over the successful UEs with a(i) in bin b
 *   timer_sum[b]    sum of timer over the same UEs
 *   done[b]         successful UEs with c(i) in bin b   (c(i) can exceed time_exit by up to 6)
 * A UE whose bin index is >= bins counts in the scalars and in the matching overflow counter, and in no bin of that axis.  Integers only: device, host,
 * forked workers and ranks merge exactly in any order.
 * PRACH_VARIANT_BETA_C and PRACH_VARIANT_WITHNOMA_C only, in both RNG modes: a NOMA_C cfg is PRACH_ERR_UNSUPPORTED, before anything is launched.  NOMA.c
 * does log the txTime of the successful Msg3 (c(i) = txTime + 6 holds there too), but its records tell arrival by the sector, have a fourth outcome and give
 * other meanings to three words: this menu must not be let loose on them.  NOMA.c has a menu of its own, the NOMA block below (prach_run_trials_noma_census). */
#define PRACH_TIMELINE_MAX_BINS 65536      /* Uniform traffic at 1 ms: 60 006 bins */

typedef struct prach_timeline_spec {
    int32_t bins;      /* 1 .. PRACH_TIMELINE_MAX_BINS */
    int32_t bin_ms;    /* >= 1 */
    int32_t ngroups;   /* number of output timelines */
    int32_t reserved;  /* 0 */
} prach_timeline_spec;

typedef struct prach_timeline {      /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                    /* sum of their nUE */
    uint64_t arrived;                /* UEs with active != -1 */
    uint64_t success;                /* UEs with msg4Flag == 1 */
    uint64_t restarted;              /* successful UEs whose last cycle did not start at their arrival */
    uint64_t arrival_overflow;       /* arrived UEs with a(i) >= bins * bin_ms (in no bin of arrivals; the successful ones in no bin of success, sojourn_sum, timer_sum) */
    uint64_t done_overflow;          /* successful UEs with c(i) >= bins * bin_ms (in no bin of done) */
    uint64_t sojourn_sum, timer_sum; /* over the successful UEs, unbinned */
    int64_t  done_max;               /* the largest c(i); -1 if success == 0 */
} prach_timeline;

/* prach_run_trials plus the timelines, with the contract of prach_run_trials_dist: trial k is added to group group[k] (group == NULL: trial k is group k and
 * ngroups must equal n); tl[ngroups] and the five series [ngroups * bins] are caller-owned and OVERWRITTEN; a trial whose final status is not PRACH_OK
 * contributes nothing; a trial the engine reruns contributes once, from the launch whose result is kept.  prach::timeline_kernel (csrc/prach_timeline.hip)
 * reduces the per-UE log records the simulation kernels write ON THE DEVICE: the engine lays them out for every trial of such a call and copies out only
 * the ones the caller asked for (ue_logs as in prach_run_trials), so the arena of the call grows by 64 bytes per UE.
 * PRACH_ERR_ARG: a NULL output, a bin count or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED: any NOMA_C cfg; 5 * ngroups * bins > 2^27 words (1 GiB of device buffer). */
int prach_run_trials_timeline(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                              const prach_timeline_spec *spec, const int32_t *group, prach_timeline *tl, uint64_t *arrivals, uint64_t *success,
                              uint64_t *sojourn_sum, uint64_t *timer_sum, uint64_t *done);

/* Sojourn distribution by arrival time per trial group, built on the device: the histogram of the time from a UE's arrival to its Msg4 — the access-delay
 * CDF of TR 37.868, which prach_dist cannot give (its `timer` is the length of the LAST attempt cycle) and prach_timeline gives only as a sum per bin —
 * by the stretch of the simulation the UE arrived in.  a(i), c(i), ARRIVED, successful and RESTARTED are those of the timeline block above.  For UE i:
 *   arrival row  r = a(i) / arrival_bin_ms          sojourn  s = c(i) - a(i)          delay bin  d = s / delay_bin_ms
 *   an arrived UE with r < arrival_bins adds 1 to row_arrived[r], otherwise to arrival_overflow (it is in no row)
 *   a successful UE with r < arrival_bins adds 1 to hist[r][d] if d < delay_bins, otherwise to row_delay_overflow[r]
 *   the scalars count every successful UE, whether or not its row is in range
 * arrival_bins = 1 with arrival_bin_ms >= maxTime is the pooled CDF: the counterpart, for the time since arrival, of the `timer` histogram of prach_dist.
 * Integers only: device, host, forked workers and ranks merge exactly in any order.  Beta.c and RandomAccessWithNOMA.c only, like the timeline. */
#define PRACH_SOJOURN_MAX_ARRIVAL_BINS 4096
#define PRACH_SOJOURN_MAX_DELAY_BINS   16384

typedef struct prach_sojourn_spec {
    int32_t arrival_bins;    /* 1 .. PRACH_SOJOURN_MAX_ARRIVAL_BINS rows */
    int32_t arrival_bin_ms;  /* >= 1; row r covers arrivals in [r * arrival_bin_ms, (r + 1) * arrival_bin_ms) */
    int32_t delay_bins;      /* 1 .. PRACH_SOJOURN_MAX_DELAY_BINS */
    int32_t delay_bin_ms;    /* >= 1 */
    int32_t ngroups;         /* number of output histograms */
    int32_t reserved;        /* 0 */
} prach_sojourn_spec;

typedef struct prach_sojourn {       /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                    /* sum of their nUE */
    uint64_t arrived;                /* UEs with active != -1 */
    uint64_t success;                /* UEs with msg4Flag == 1 */
    uint64_t restarted;              /* successful UEs whose last cycle did not start at their arrival */
    uint64_t arrival_overflow;       /* arrived UEs with a(i) >= arrival_bins * arrival_bin_ms: in no row */
    uint64_t delay_overflow;         /* successful UEs, in a row or not, with sojourn >= delay_bins * delay_bin_ms */
    uint64_t sojourn_sum;            /* over all successful UEs, unbinned */
    int64_t  sojourn_max;            /* the largest sojourn; -1 if success == 0 */
} prach_sojourn;

/* prach_run_trials plus the sojourn histograms, with the contract of prach_run_trials_timeline: trial k is added to group group[k] (group == NULL: trial k is
 * group k and ngroups must equal n); sj[ngroups], hist[ngroups][arrival_bins][delay_bins], row_arrived[ngroups][arrival_bins] and
 * row_delay_overflow[ngroups][arrival_bins] are caller-owned and OVERWRITTEN; a trial whose final status is not PRACH_OK contributes nothing; a trial the
 * engine reruns contributes once, from the launch whose result is kept.  prach::sojourn_kernel (csrc/prach_sojourn.hip) reduces the per-UE log records the
 * simulation kernels write ON THE DEVICE: the engine lays them out for every trial of such a call and copies out only the ones the caller asked for, so
 * the arena of the call grows by 64 bytes per UE.
 * PRACH_ERR_ARG: a NULL output, a bin count or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED: any NOMA_C cfg (before anything is launched); ngroups * arrival_bins * (delay_bins + 2) > 2^27 words (1 GiB of device buffer). */
int prach_run_trials_sojourn(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                             const prach_sojourn_spec *spec, const int32_t *group, prach_sojourn *sj, uint64_t *hist, uint64_t *row_arrived,
                             uint64_t *row_delay_overflow);

/* Outcome cross-tabulation per trial group, built on the device: a two-axis table over a FIXED MENU of per-UE quantities, with a choice of WHICH UEs enter.
 * The other reductions describe the UEs a trial served; this one also says what became of the ones it left behind.  Everything comes from the 64-byte log
 * record, the arrival schedule and the trial's `steps`: nothing new is simulated.  a(i), c(i), ARRIVED and successful are those of the timeline block above;
 * E = min(prach_result.steps, maxTime) is the subframe the run ended at.  Every UE is in exactly one CLASS, the bits of `who`:
 *   PRACH_XTAB_IDLE      active == -1 (not arrived)
 *   PRACH_XTAB_SERVED    arrived and msg4Flag == 1
 *   PRACH_XTAB_UNSERVED  arrived and not served
 * `who` is a non-empty subset; a UE outside it counts in `ues` and in its class scalar only.  FIELDS: the value of UE i, or UNDEFINED for it:
 *   0 ONE         0                              every UE
 *   1 ARRIVAL     a(i)                           arrived
 *   2 SOJOURN     c(i) - a(i)                    served
 *   3 COMPLETION  c(i)                           served
 *   4 TIMER       logged timer                   arrived (unserved: the time since its current cycle began)
 *   5 PTC         logged preambleTxCounter       arrived (the transmissions of the current cycle)
 *   6 FAILCOUNT   logged failCount               arrived (cycles started over; Beta.c logs 0)
 *   7 AGE         E - a(i)                       arrived (the time in the system when the run ended)
 *   8 STATE       0 idle, 1 served, then for the unserved: 2 active == 1 && nowBackoff > 0 (in a backoff), 3 active == 1 && nowBackoff <= 0 (in a RAR
 *                 window), 4 active == 2 && connectionRequest < 48 (granted, Msg3 pending), 5 active == 2 && connectionRequest >= 48 (waiting out the
 *                 Msg3 timeout), 6 anything else (no trial produces it)                          every UE
 * ONE RULE for bad values: a NEGATIVE value is UNDEFINED (idle UEs log timer = txTime = -1; an E below an arrival makes that UE's AGE undefined — nothing is
 * refused and nothing is clipped).
 * An axis has `bins` regular bins of `width` (bin b covers [b * width, (b + 1) * width)) plus ONE OVERFLOW BIN at index `bins`; the table of a group is
 * (row_bins + 1) x (col_bins + 1) 64-bit cells, row-major.  A UE in `who` whose row and column values are both defined adds 1 to exactly one cell; one with an
 * undefined value adds 1 to `undefined` and to no cell: sum(cells) + undefined == selected, always.  Integers only: device, host, forked workers and ranks
 * merge exactly in any order.  Beta.c and RandomAccessWithNOMA.c only, like the timeline.
 * A fine ARRIVAL x SOJOURN table remains prach_run_trials_sojourn's job (its kernel windows such a table by arrival row; this one does not). */
#define PRACH_XTAB_SERVED   1
#define PRACH_XTAB_UNSERVED 2
#define PRACH_XTAB_IDLE     4
#define PRACH_XTAB_MAX_BINS 65536
enum { PRACH_XTAB_ONE = 0, PRACH_XTAB_ARRIVAL, PRACH_XTAB_SOJOURN, PRACH_XTAB_COMPLETION, PRACH_XTAB_TIMER, PRACH_XTAB_PTC, PRACH_XTAB_FAILCOUNT, PRACH_XTAB_AGE,
       PRACH_XTAB_STATE, PRACH_XTAB_NFIELDS };

typedef struct prach_xtab_spec {
    int32_t who;                              /* PRACH_XTAB_* class bits, not 0 */
    int32_t row_field, row_width, row_bins;   /* a field id, width >= 1, 1 .. PRACH_XTAB_MAX_BINS regular bins */
    int32_t col_field, col_width, col_bins;
    int32_t ngroups;                          /* number of output tables */
    int32_t reserved[2];                      /* 0 */
} prach_xtab_spec;

typedef struct prach_xtab {          /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                    /* sum of their nUE */
    uint64_t idle, served, unserved; /* the three classes, counted regardless of `who`: idle + served + unserved == ues */
    uint64_t selected;               /* UEs whose class is in `who` */
    uint64_t binned, undefined;      /* ... of which: in a cell (overflow cells included) / with an undefined row or column value */
    uint64_t row_sum, col_sum;       /* sums of the two values over the binned UEs, unbinned */
    int64_t  row_max, col_max;       /* the largest of each over the binned UEs; -1 if binned == 0 */
} prach_xtab;

/* prach_run_trials plus the cross-tabulation, with the contract of prach_run_trials_sojourn: trial k is added to group group[k] (group == NULL: trial k is
 * group k and ngroups must equal n); xt[ngroups] and cells[ngroups][row_bins + 1][col_bins + 1] are caller-owned and OVERWRITTEN; a trial whose final status
 * is not PRACH_OK contributes nothing; a trial the engine reruns contributes once, from the launch whose result is kept.  prach::xtab_kernel
 * (csrc/prach_xtab.hip) reduces the per-UE log records the simulation kernels write ON THE DEVICE, as the timeline does.
 * PRACH_ERR_ARG: a NULL output, an unknown field or class bit, an empty `who`, a bin count or width out of range, a non-zero reserved word, a group id out of
 * range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED: any NOMA_C cfg (before anything is launched); ngroups * (row_bins + 1) * (col_bins + 1) > 2^27 words (1 GiB of device buffer). */
int prach_run_trials_xtab(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_xtab_spec *spec,
                          const int32_t *group, prach_xtab *xt, uint64_t *cells);

/* Per-trial summary, built on the device: ONE row per TRIAL — counts, sums, maxima and EXACT order statistics of the sojourn, of `timer` and of
 * preambleTxCounter over the trial's successful UEs — so that the spread from seed to seed of any of them, a percentile included, can be stated
 * (prach_summary_stats).  The pooled reductions above cannot give that: they add trials into shared bins.  a(i), c(i), ARRIVED, successful and RESTARTED are
 * those of the timeline block above.
 * THE DEFINITION of a level: for a quantity X over the n = success successful UEs of ONE trial and a level m in permille (1..1000), the rank is
 *   r = max(1, (n * m + 999) / 1000)      in 64-bit integers
 * and the value is the r-th smallest X.  No bins, no interpolation.  The rule is deliberately integer; at m = 500 it coincides with the ceil(q * n) of
 * prach_sojourn_quantile (0.5 is exact in binary); no wider equivalence is claimed.
 * Beta.c and RandomAccessWithNOMA.c only, like the timeline. */
#define PRACH_SUMMARY_MAX_Q 8
typedef struct prach_summary_spec { int32_t nq; int32_t permille[PRACH_SUMMARY_MAX_Q]; int32_t reserved[3]; } prach_summary_spec; /* nq 1..8, levels 1..1000 */
typedef struct prach_trial_summary {      /* one per TRIAL */
    int32_t status, nUE, arrived, success, restarted, range_errors;
    int64_t sojourn_sum, timer_sum, ptc_sum;             /* over the successful UEs */
    int32_t sojourn_max, timer_max, ptc_max;             /* -1 if success == 0 */
    int32_t q[3][PRACH_SUMMARY_MAX_Q];                   /* [sojourn, timer, preambleTxCounter][level]; -1 if success == 0 or level unused */
} prach_trial_summary;
typedef struct prach_stat { uint64_t n; double mean, sd, sem, min, max; } prach_stat;

/* prach_run_trials plus one summary row per trial: rows[n] is caller-owned and OVERWRITTEN.  Row k carries the final status of trial k and cfgs[k].nUE; unless
 * that status is PRACH_OK everything else in it is 0, the maxima and levels -1.  A trial the engine reruns is written once, by the launch whose result is
 * kept.  prach::summary_kernel (csrc/prach_summary.hip) selects the order statistics from the per-UE log records the simulation kernels write ON THE DEVICE,
 * one workgroup per trial; it handles values 0 .. prach_summary_max_value().  range_errors counts the successful UEs with a value outside that range (no
 * trial produces one): the levels of that quantity are -1 then and the call returns PRACH_ERR_INTERNAL.
 * PRACH_ERR_ARG: a NULL output or spec, nq or a level out of range, a non-zero reserved word; PRACH_ERR_UNSUPPORTED: any NOMA_C cfg (before anything is
 * launched). */
int prach_run_trials_summary(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                             const prach_summary_spec *spec, prach_trial_summary *rows);

/* Pick per trial, selected on the device: WHICH UEs stand behind a count — per TRIAL the k UEs that match a predicate over the menu of the cross-tabulation
 * above, as records, and the exact number of matches.  The other reductions answer "how many" and "how long"; the only other route to the individuals is
 * every per-UE log over the bus and a filter on the host.  `who` is the PRACH_XTAB_* class bits (the same three classes); the value of a field, a(i), c(i)
 * and E = min(steps, maxTime) are exactly those of the xtab block, with its ONE RULE: a negative value is UNDEFINED.
 *   selected   the UEs whose class is in `who`
 *   a clause {field, lo, hi} HOLDS for a UE when the field's value v is defined and lo <= v <= hi (inclusive; lo >= 0), and FAILS when v is defined and
 *              outside; the values a UE NEEDS are those of its clauses and, under LARGEST / SMALLEST, that of key_field
 *   matched    the selected UEs all of whose needed values are defined and all of whose clauses hold; exact, whatever k is
 *   undefined  the selected UEs of which no clause fails and at least one needed value is undefined (they fail to match only for that)
 * ORDER: which of the matches are returned, and in which order:
 *   PRACH_PICK_BY_INDEX   the first k matches in UE-index order; key_field must be PRACH_XTAB_ONE (0), every row's `key` is 0, threshold -1, ties_left_out 0
 *   PRACH_PICK_LARGEST    the k matches that come first when sorted by descending key (the value of key_field), equal keys in ascending UE index, in that
 *                         order; threshold is the key of the last stored row (-1: none), ties_left_out the matches with key == threshold that are not stored
 *   PRACH_PICK_SMALLEST   the mirror image: ascending key, equal keys in ascending UE index
 * stored = min(matched, k); the rows behind `stored` are zero.  A row is the UE's 64-byte log record, its arrival a(i) (-1 for an idle UE) and its key.
 * Keys are RANKED in the range 0 .. prach_summary_max_value() (65 535), like the summary's order statistics; a match with a key outside it is counted in
 * range_errors.  No trial produces one: SOJOURN, TIMER and PTC are bounded as csrc/prach_summary.hip states, ARRIVAL, COMPLETION and AGE by the 60 000 + 6
 * subframes of the longest trial, FAILCOUNT by one cycle per subframe, STATE by 6.  When range_errors is non-zero the trial's rows are void (zero, stored 0,
 * threshold -1) and the call returns PRACH_ERR_INTERNAL, as for the summary.
 * The output is defined per trial: it does not depend on how a call is split into launches, on reruns, or on how trials are dealt to devices and ranks.
 * Beta.c and RandomAccessWithNOMA.c only, like the timeline. */
#define PRACH_PICK_MAX_K        4096
#define PRACH_PICK_MAX_CLAUSES  4
enum { PRACH_PICK_BY_INDEX = 0, PRACH_PICK_LARGEST = 1, PRACH_PICK_SMALLEST = 2 };
typedef struct prach_pick_clause { int32_t field, lo, hi; } prach_pick_clause; /* a PRACH_XTAB_* field id, 0 <= lo <= hi */
typedef struct prach_pick_spec {
    int32_t who;                                        /* PRACH_XTAB_* class bits, not 0 */
    int32_t nclauses;                                   /* 0 .. PRACH_PICK_MAX_CLAUSES; the clauses behind it must be zero */
    prach_pick_clause clause[PRACH_PICK_MAX_CLAUSES];
    int32_t order, key_field;                           /* PRACH_PICK_*; a PRACH_XTAB_* field id (BY_INDEX: 0) */
    int32_t k;                                          /* 1 .. PRACH_PICK_MAX_K rows per trial */
    int32_t reserved;                                   /* 0 */
} prach_pick_spec;
typedef struct prach_pick_row { /* 80 bytes, 8-byte aligned */
    __attribute__((aligned(8))) prach_ue_log log;
    int32_t arrival;            /* a(i); -1 for an idle UE */
    int32_t key;                /* the value of key_field (BY_INDEX: 0) */
    int32_t pad[2];             /* 0 */
} prach_pick_row;
typedef struct prach_pick {     /* one per TRIAL */
    int32_t status, nUE, selected, matched, stored, undefined, range_errors, threshold, ties_left_out;
} prach_pick;

/* prach_run_trials plus the pick: picks[n] and rows[n * spec->k] (trial t's rows at rows + t * k) are caller-owned and OVERWRITTEN.  picks[t] carries the final
 * status of trial t and cfgs[t].nUE; unless that status is PRACH_OK everything else in it is 0 (threshold -1) and its rows are zero.  A trial the engine reruns
 * is written once, by the launch whose result is kept.  prach::pick_kernel (csrc/prach_pick.hip) selects from the per-UE log records the simulation kernels
 * write ON THE DEVICE, one workgroup per trial, and leaves a trial's rows in UE-index order; the engine sorts the at most k rows of a trial into the defined
 * order on the host.
 * PRACH_ERR_ARG: a NULL output or spec, an unknown field, class bit or order, an empty `who`, k or nclauses out of range, lo < 0 or lo > hi, a non-zero unused
 * clause, a key field other than 0 with BY_INDEX, a non-zero reserved word; PRACH_ERR_UNSUPPORTED: any NOMA_C cfg (before anything is launched);
 * n * k * 10 + n * 8 > 2^27 words (1 GiB of device buffer). */
int prach_run_trials_pick(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_pick_spec *spec,
                          prach_pick *picks, prach_pick_row *rows);

/* Per-UE columns, computed on the device: the menu of the cross-tabulation above for EVERY UE of every trial, as plain int32 columns — the escape hatch for
 * a question outside the fixed kinds (a correlation, a survival curve, a quantile by two conditions).  The other route to the same values is 64 bytes per UE
 * over the bus and a restatement of a(i), the classes and the STATE rule on the host; this one moves 4 bytes per asked-for field, or nothing at all: the
 * columns go to the host, or into DEVICE memory the caller owns (a torch tensor), where any further reduction runs.
 * A FIELD is a PRACH_XTAB_* id (0 .. 8) or PRACH_COL_RAW + w, w = 0 .. 15: word w of the UE's prach_ue_log, exactly as logged.  A menu field holds the
 * menu's value with E = min(steps, maxTime), and -1 where the menu says UNDEFINED (its ONE RULE: a negative value is undefined, so is a field outside the
 * classes it is defined for); every menu value of a trial fits int32 (csrc/prach_columns.hip states the bound).  A field may be named twice.
 * LAYOUT: column c of UE i of trial k is out[c * rows_cap + hdr[k].offset + i]; hdr[k].offset is the sum of cfgs[j].nUE over j < k, whatever their status.
 * A trial whose final status is not PRACH_OK has -1 in every word of every column and its status in its header.  Words at rows >= the sum of all nUE are
 * not touched.  Beta.c and RandomAccessWithNOMA.c only, like the timeline. */
#define PRACH_COL_MAX 16
#define PRACH_COL_RAW 16   /* field PRACH_COL_RAW + w, w = 0..15: word w of the UE's prach_ue_log, exactly as logged */
#define PRACH_COL_MAX_WORDS (1ull << 31) /* ncols * rows_cap at most: 8 GiB of columns (the 1000-trial grid, 55 M UEs, with 16 columns is 0.9 x 2^30 words) */
typedef struct prach_columns_spec { int32_t ncols; int32_t field[PRACH_COL_MAX]; int32_t reserved[3]; } prach_columns_spec; /* ncols 1..16; the fields behind it are ignored */
typedef struct prach_columns {            /* one per TRIAL */
    int32_t status, nUE; uint64_t offset; /* first row of this trial: the sum of cfgs[j].nUE over j < k, whatever their status */
    int32_t idle, served, unserved, reserved; /* the three classes, counted by the kernel: idle + served + unserved == nUE; 0 unless status is PRACH_OK */
} prach_columns;

/* prach_run_trials plus the columns: hdr[n] and out[ncols * rows_cap] are caller-owned; hdr is OVERWRITTEN, and so are the rows [0, sum of nUE) of every
 * column.  A trial the engine reruns — the calendar rerun, a call split by its memory budget, the fallback ladder, a timeout — is written by the ONE launch
 * whose result is kept; the output does not depend on how a call is split.  prach::columns_kernel (csrc/prach_columns.hip) writes into a buffer of the
 * engine's, which is filled with -1 once in front of the first launch and copied out once at the end of the call.
 * prach_run_trials_columns_device: the same with dev_out in DEVICE memory of the engine's device (hipPointerGetAttributes must say so): the kernel writes
 * straight into it, nothing but the headers crosses the bus.  The memory must be made by the HIP runtime this library is linked to (one process, one
 * runtime: README.md), and work queued on it on other streams must have completed.
 * Refused before anything is launched or written —
 * PRACH_ERR_ARG: a NULL spec, header or destination, ncols outside 1 .. PRACH_COL_MAX, a field outside the menu and outside 16 .. 31, a non-zero reserved
 * word, rows_cap below the sum of all nUE; _device: a destination that is not device memory of the engine's device;
 * PRACH_ERR_UNSUPPORTED: any NOMA_C cfg; ncols * rows_cap > PRACH_COL_MAX_WORDS. */
int prach_run_trials_columns(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_columns_spec *spec,
                             prach_columns *hdr, int32_t *out, uint64_t rows_cap);
int prach_run_trials_columns_device(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                    const prach_columns_spec *spec, prach_columns *hdr, void *dev_out, uint64_t rows_cap);
/* THE DEFINITION prach::columns_kernel equals, integer for integer: the columns of ONE trial from its per-UE log; steps is the trial's prach_result.steps.
 * Column c of UE i at out[c * stride + i] (stride >= nUE).  PRACH_ERR_ARG: a bad spec, a NULL pointer, nUE != cfg->nUE, stride < nUE;
 * PRACH_ERR_UNSUPPORTED: a NOMA_C cfg. */
int prach_columns_from_logs(const prach_columns_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, int32_t *out, uint64_t stride);
int prach_columns_tile_ues(void); /* UEs of one trial that one workgroup of prach::columns_kernel writes (tests place sizes around it) */

/* THE NOMA MENU: NOMA.c's own outcome census and per-UE columns, on the device.  PRACH_VARIANT_NOMA_C trials only; the menu above stays what it is and keeps
 * refusing them.  Everything comes from the 64-byte log record of a NOMA.c trial, the arrival schedule and the trial's `steps`.
 *   a(i)  the timeline block's arrival: the same schedule and the same search
 *   E     min(prach_result.steps, maxTime)
 *   c(i)  txTime + 6.  A NOMA.c success happens in the subframe time == txTime, leaves txTime alone and adds 6 to `timer` (NOMA.c:499-546), and `timer` was
 *         zeroed at activation and at a Msg3 timeout: c(i) - timer is the start of the last cycle, as in the other two programs.
 * What differs: `active` cannot tell an idle UE from a served one (both log 0), so ARRIVED is `preambleChange != -1` (NOMA.c logs the sector there); a UE whose
 * msg1ReTx reaches maxMsg1ReTx is DROPPED for good (RaFailed); failCount = RaFailed | msg3Faile << 16, maxRarCounter = msg1ReTx, connectionRequest = msg3Wait.
 * CLASSES, by precedence, the bits of `who`:
 *   PRACH_NOMA_IDLE     preambleChange == -1
 *   PRACH_NOMA_SERVED   arrived and msg4Flag == 1
 *   PRACH_NOMA_DROPPED  arrived, not served, (failCount & 0xffff) != 0
 *   PRACH_NOMA_PENDING  arrived, neither served nor dropped
 * FIELDS: the value of UE i, or UNDEFINED outside the classes named:
 *    0 ONE         0                                        every UE
 *    1 ARRIVAL     a(i)                                     arrived
 *    2 SOJOURN     c(i) - a(i)                              served
 *    3 COMPLETION  c(i)                                     served
 *    4 TIMER       logged timer (a dropped UE logs 0)       arrived
 *    5 PTC         logged preambleTxCounter (nTxPreamble)   arrived
 *    6 RETX        logged maxRarCounter (msg1ReTx)          arrived
 *    7 MSG3FAIL    failCount >> 16 (msg3Faile)              arrived
 *    8 AGE         E - a(i)                                 arrived
 *    9 STATE       0 idle, 1 served, 2 dropped, then for the pending: 3 active == 1 && nowBackoff > 0 (in a backoff), 4 active == 1 && nowBackoff <= 0 &&
 *                  txTime >= E (its transmit subframe is ahead), 5 active == 1 && nowBackoff <= 0 && txTime < E (STRANDED: its transmit subframe has
 *                  passed), 6 active == 2 && connectionRequest == 0 (Msg3 pending), 7 active == 2 && connectionRequest != 0 (waiting out a Msg3
 *                  timeout), 8 anything else (no trial produces it)                                         every UE
 *   10 SECTOR      logged preambleChange, 0..5              arrived
 *   11 PREAMBLE    logged preamble                          arrived
 *   12 LOST        SOJOURN - TIMER: arrival to the start of the last cycle; 0 iff the UE never started over   served
 *                  (undefined where SOJOURN or TIMER is, and where the difference is negative)
 * STATE 5 IS FINAL.  NOMA.c moves a UE with active == 1 in two places, the collision detection (NOMA.c:325-447, the oracle's noma_oracle.c:203) and
 * msg2Results (:325 there); both ask txTime == time + 1.  The Msg3 step (:331) asks txTime == time.  All three need txTime >= time, and time only grows: a UE
 * with active == 1, nowBackoff <= 0 and txTime below the current subframe is never touched again, only its timer ticks to the end of the run.  NOMA.c reports
 * no such UE; the backoff's off-by-one makes them.
 * ONE RULE as in the xtab block: a NEGATIVE value is UNDEFINED, nothing is refused, nothing is clipped.  Every menu value of a trial fits int32
 * (csrc/prach_noma_menu.h states the bounds).  The channel gain is not a FIELD of the menu (the field count is fixed); it is the axis of a kind of its own,
 * prach_run_trials_noma_gain below.  With Philox it is also available per UE through prach_noma_activation_table and prach_noma_gain_levels; in the
 * reference's stream it exists only inside the launch.
 * PRACH_RNG_GLIBC trials of NOMA_C are not wired to the device calls below (their launches lay out no job the menu's kernels read): the calls refuse them, and
 * prach_run_trials with logs plus the host definitions serves them. */
#define PRACH_NOMA_SERVED  1
#define PRACH_NOMA_PENDING 2
#define PRACH_NOMA_IDLE    4
#define PRACH_NOMA_DROPPED 8
enum { PRACH_NOMA_ONE = 0, PRACH_NOMA_ARRIVAL, PRACH_NOMA_SOJOURN, PRACH_NOMA_COMPLETION, PRACH_NOMA_TIMER, PRACH_NOMA_PTC, PRACH_NOMA_RETX, PRACH_NOMA_MSG3FAIL,
       PRACH_NOMA_AGE, PRACH_NOMA_STATE, PRACH_NOMA_SECTOR, PRACH_NOMA_PREAMBLE, PRACH_NOMA_LOST, PRACH_NOMA_NFIELDS };

typedef struct prach_noma_census {            /* one per group */
    uint64_t trials;                          /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                             /* sum of their nUE */
    uint64_t idle, served, dropped, pending;  /* the four classes, counted regardless of `who`: idle + served + dropped + pending == ues */
    uint64_t selected;                        /* UEs whose class is in `who` */
    uint64_t binned, undefined;               /* ... of which: in a cell (overflow cells included) / with an undefined row or column value */
    uint64_t row_sum, col_sum;                /* sums of the two values over the binned UEs, unbinned */
    int64_t  row_max, col_max;                /* the largest of each over the binned UEs; -1 if binned == 0 */
} prach_noma_census;

/* prach_run_trials plus the NOMA census: the contract of prach_run_trials_xtab word for word (groups, OVERWRITTEN outputs, a rerun trial counted once), with a
 * prach_xtab_spec whose `who` is PRACH_NOMA_* class bits and whose fields are PRACH_NOMA_* ids; the cells are laid out as xtab's are: sum(cells) + undefined
 * == selected.  prach::noma_census_kernel (csrc/prach_noma_census.hip) reduces the log records on the device; engine option "xtab_scheme" applies.
 * PRACH_ERR_ARG: the argument cases of prach_run_trials_xtab, with NOMA's ids and bits;
 * PRACH_ERR_UNSUPPORTED, before anything is launched: any cfg that is not NOMA_C; any NOMA_C cfg with rng_mode == PRACH_RNG_GLIBC; ngroups * (row_bins + 1) *
 * (col_bins + 1) > 2^27 words.  PRACH_FLAG_NOMA_NONSECTOR is accepted. */
int prach_run_trials_noma_census(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_xtab_spec *spec,
                                 const int32_t *group, prach_noma_census *cs, uint64_t *cells);

/* Per-UE columns of NOMA_C trials: the contract of prach_run_trials_columns and prach_run_trials_columns_device (layout, rows_cap, -1 for undefined,
 * PRACH_COL_RAW + w, the device-pointer check, refusals before anything is written) with PRACH_NOMA_* field ids; the refusals are the census's.
 * prach::noma_columns_kernel (csrc/prach_noma_census.hip) writes them. */
typedef struct prach_noma_columns {           /* one per TRIAL */
    int32_t status, nUE; uint64_t offset;     /* first row of this trial: the sum of cfgs[j].nUE over j < k, whatever their status */
    int32_t idle, served, dropped, pending;   /* the four classes, counted by the kernel: their sum is nUE; 0 unless status is PRACH_OK */
} prach_noma_columns;
int prach_run_trials_noma_columns(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                  const prach_columns_spec *spec, prach_noma_columns *hdr, int32_t *out, uint64_t rows_cap);
int prach_run_trials_noma_columns_device(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                         const prach_columns_spec *spec, prach_noma_columns *hdr, void *dev_out, uint64_t rows_cap);

/* NOMA menu, host side (no device needed; both RNG modes).  cs and cells [row_bins + 1][col_bins + 1]: ONE group.
 * prach_noma_census_accumulate_logs ADDS one trial's per-UE log to a group: THE DEFINITION prach::noma_census_kernel equals, integer for integer.  steps is the
 * trial's prach_result.steps.  PRACH_ERR_UNSUPPORTED: a cfg that is not NOMA_C.  PRACH_ERR_ARG: a bad spec or cfg, nUE != cfg->nUE (no log content is refused).
 * _merge adds counts and sums and takes the maxima; _format_csv writes prach_xtab_format_csv's lines.  prach_xtab_quantile reads the cells of a census with a
 * spec of the same widths and bin counts. */
int prach_noma_census_accumulate_logs(const prach_xtab_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_noma_census *cs,
                                      uint64_t *cells);
void prach_noma_census_merge(const prach_xtab_spec *, prach_noma_census *into, uint64_t *cells_into, const prach_noma_census *from, const uint64_t *cells_from);
size_t prach_noma_census_format_csv(const prach_xtab_spec *, const prach_noma_census *, const uint64_t *cells, const char *label, char *buf, size_t cap);
int prach_noma_census_tile_ues(void); /* UEs of one trial that one workgroup of prach::noma_census_kernel reduces (tests place sizes around it) */
/* THE DEFINITION prach::noma_columns_kernel equals, integer for integer: prach_columns_from_logs with the NOMA menu.  PRACH_ERR_UNSUPPORTED: not a NOMA_C cfg. */
int prach_noma_columns_from_logs(const prach_columns_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, int32_t *out, uint64_t stride);

/* NOMA.c's channel trace per trial group: per access slot and sector, how many preambles were sent, how many stood alone, how many bins collided, how many
 * power-domain pairs the grouping formed and how many of those decoded one UE only — recorded by prach::noma_kernel WHILE IT RUNS and reduced on the device.
 * Like prach_trace it is no function of the per-UE state a trial leaves behind, so there is no _accumulate_logs form.  Per slot s (subframe s * accessTime) and
 * sector c of a trial, in NOMA.c's own terms:
 *   tx        transmitters gathered by preambleSectorCollisionDetection (NOMA.c:206-212): the sum of the sector's (sector, preamble) bin counts
 *   used      bins with at least one transmitter;  singles  bins with exactly one (NOMA.c:214-243: `count`);  used - singles = COLLIDED bins
 *   granted   UEs whose msg2 the slot sets (count, where count <= nGrantUL)
 *   pairs     power-domain pairs that received a grant (NOMA.c:279-286);  pair_one  of those, the pairs of which only one UE decoded (the first decode draw
 *             below 0.3; under PRACH_FLAG_NOMA_NONSECTOR too, where no second draw follows).  UEs granted through NOMA: 2 * pairs - pair_one
 * Under PRACH_FLAG_NOMA_NONSECTOR there is one group: it is sector 0 and the other five stay zero.  A trial's rows cover the slots whose subframe lies in
 * [0, steps); a (slot, sector) without a transmitter is all zero.  Slot s falls into bin (s * accessTime) / bin_ms; a slot at or behind bins * bin_ms counts in
 * the scalars and in no bin, its tx in overflow_tx.  Integers only: device, host, forked workers and ranks merge exactly in any order.  The six series are
 * [ngroups][6 sectors][bins] each, in the order tx, used, singles, granted, pairs, pair_one. */
#define PRACH_NOMA_TRACE_SERIES 6
typedef struct prach_noma_trace_spec {
    int32_t bins;      /* 1 .. PRACH_TRACE_MAX_BINS */
    int32_t bin_ms;    /* >= 1 */
    int32_t ngroups;   /* number of output traces */
    int32_t reserved;  /* 0 */
} prach_noma_trace_spec;

typedef struct prach_noma_trace {    /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t slots;                  /* access slots read: the sum of ceil(steps / accessTime) */
    uint64_t tx, used, singles, granted, pairs, pair_one; /* over all their slots and sectors, unbinned */
    uint64_t overflow_tx;            /* tx in slots at or behind bins * bin_ms (in no bin) */
    int64_t  tx_max;                 /* the largest `tx` of one (slot, sector) of one trial; -1 without slots */
} prach_noma_trace;

/* prach_run_trials plus the channel traces, with the contract of prach_run_trials_noma_census (groups, OVERWRITTEN outputs, a rerun trial counted once, at most
 * one reduction per call); tr[ngroups] and series[q][ngroups * 6 * bins] are caller-owned.  prach::noma_kernel writes one 32-byte row per (slot, sector) ON THE
 * DEVICE (the arena of the call grows by 192 bytes x ceil(maxTime / accessTime) per trial) and prach::noma_trace_kernel (csrc/prach_noma_trace.hip) reduces
 * them there; engine option "trace_scheme" applies.  Results and logs are those of the same prach_run_trials call.
 * PRACH_ERR_ARG: a NULL output, a bin count or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED, before anything is launched: any cfg that is not NOMA_C; any NOMA_C cfg with rng_mode == PRACH_RNG_GLIBC; 36 * ngroups * bins > 2^27
 * words. */
int prach_run_trials_noma_trace(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                const prach_noma_trace_spec *spec, const int32_t *group, prach_noma_trace *tr, uint64_t *const series[6]);
/* host side, ONE group (series[q]: [6][bins]): _merge adds counts and takes the maximum; _format_csv writes "label,series,sector,t_ms,count" for every
 * non-zero (bin, sector), an all-sectors line "label,series,all,t_ms,count" for every non-zero bin, and "label,tx,all,overflow,count" if overflow_tx != 0;
 * returns the text's length (written in full only if it fits cap, then 0-terminated). */
void prach_noma_trace_merge(const prach_noma_trace_spec *, prach_noma_trace *into, uint64_t *const into_series[6], const prach_noma_trace *from, const uint64_t *const from_series[6]);
size_t prach_noma_trace_format_csv(const prach_noma_trace_spec *, const prach_noma_trace *, const uint64_t *const series[6], const char *label, char *buf, size_t cap);
int prach_noma_trace_tile_rows(void); /* (slot, sector) rows of one trial that one workgroup of prach::noma_trace_kernel reduces (tests place sizes around it) */

/* NOMA.c's timeline per trial group and SECTOR: what became of the UEs that arrived in each stretch of the simulation, and how long they waited — the other
 * half of the channel trace above, on the trace's own bins, so that tx / singles / pairs of a (sector, bin) stand next to arrivals / served / dropped / mean
 * sojourn / mean lost time of the UEs that arrived in it.  Everything is a function of the per-UE log, the arrival schedule and `steps`, so there IS an
 * _accumulate_logs form, and it is THE DEFINITION.  It uses a(i), E, c(i) = txTime + 6, the four classes and the fields of THE NOMA MENU as they stand.
 * For UE i with class cls, sector s = SECTOR, arrival bin ab = a(i) / bin_ms and completion bin db = c(i) / bin_ms:
 *   - every UE counts in its class counter (idle, served, dropped, pending): their sum is `ues`;
 *   - an arrived UE is UNDEFINED FOR THE TIMELINE if its SECTOR lies outside 0..5, or if it is served and any of SOJOURN, TIMER, COMPLETION is negative (the
 *     menu's ONE RULE).  It counts in `undefined` and in nothing else below.  No trial produces one;
 *   - every other arrived UE: ab < bins: arrivals[s][ab] += 1; otherwise arrival_overflow += 1;
 *   - dropped, with ab < bins: dropped[s][ab] += 1;
 *   - served: the scalars sojourn_sum += SOJOURN, timer_sum += TIMER, done_max = max(done_max, c(i)), restarted += LOST > 0 (as
 *     prach_noma_trial_summary.restarted), always; if ab < bins: served[s][ab] += 1, sojourn_sum[s][ab] += SOJOURN, timer_sum[s][ab] += TIMER; if db < bins:
 *     done[s][db] += 1, otherwise done_overflow += 1.
 * Pending per (sector, bin) is arrivals - served - dropped; it is not stored.  IDENTITY: sum(arrivals) + arrival_overflow + undefined == served + dropped +
 * pending.  The six series are [ngroups][6 sectors][bins] each, in the order arrivals, served, dropped, sojourn_sum, timer_sum, done: the layout of
 * prach_noma_trace's series, so the two line up index for index.  ONE DIFFERENCE from the trace: under PRACH_FLAG_NOMA_NONSECTOR the trace puts the one
 * cell-wide group into sector 0, while the timeline's sector is still the record's own word — the UE's sector, not the grouping's.
 * Integers only, 64-bit outputs: device, host, forked workers and ranks merge exactly in any order.
 * THERE IS NO NOMA SOJOURN KIND: prach_run_trials_noma_census with ARRIVAL by SOJOURN over PRACH_NOMA_SERVED is that histogram, and prach_xtab_quantile reads
 * it.  The timeline adds what no census cell holds: the sums, the by-completion axis, and both split by sector on the bins of the channel trace. */
#define PRACH_NOMA_TIMELINE_SERIES 6
typedef struct prach_noma_timeline_spec {
    int32_t bins;      /* 1 .. PRACH_TIMELINE_MAX_BINS */
    int32_t bin_ms;    /* >= 1 */
    int32_t ngroups;   /* number of output timelines */
    int32_t reserved;  /* 0 */
} prach_noma_timeline_spec;

typedef struct prach_noma_timeline { /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                    /* sum of their nUE */
    uint64_t idle, served, dropped, pending; /* the four classes: idle + served + dropped + pending == ues */
    uint64_t undefined;              /* arrived UEs that are undefined for the timeline (in no series, no overflow and no sum) */
    uint64_t restarted;              /* served, defined, LOST > 0 */
    uint64_t arrival_overflow;       /* defined arrived UEs with a(i) at or behind bins * bin_ms */
    uint64_t done_overflow;          /* defined served UEs with c(i) at or behind bins * bin_ms */
    uint64_t sojourn_sum, timer_sum; /* over the defined served UEs, unbinned */
    int64_t  done_max;               /* the largest c(i) of a defined served UE; -1 without one */
} prach_noma_timeline;

/* prach_run_trials plus the NOMA timelines, with the contract of prach_run_trials_noma_trace word for word (groups, OVERWRITTEN outputs, a rerun trial counted
 * once, at most one reduction per call); tl[ngroups] and series[q][ngroups * 6 * bins] are caller-owned.  prach::noma_timeline_kernel
 * (csrc/prach_noma_timeline.hip) reduces the log records prach::noma_kernel wrote on the device; engine option "timeline_scheme" applies.
 * PRACH_ERR_ARG: a NULL output, a bin count or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED, before anything is launched: any cfg that is not NOMA_C; any NOMA_C cfg with rng_mode == PRACH_RNG_GLIBC; 36 * ngroups * bins > 2^27
 * words.  A refusal writes nothing. */
int prach_run_trials_noma_timeline(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                   const prach_noma_timeline_spec *spec, const int32_t *group, prach_noma_timeline *tl, uint64_t *const series[6]);
/* host side (no device needed; both RNG modes), ONE group (series[q]: [6][bins]).  prach_noma_timeline_accumulate_logs ADDS one trial's per-UE log to a group:
 * THE DEFINITION prach::noma_timeline_kernel equals, integer for integer; steps is the trial's prach_result.steps.  PRACH_ERR_UNSUPPORTED: a cfg that is not
 * NOMA_C.  PRACH_ERR_ARG: a bad spec or cfg, a NULL pointer, nUE != cfg->nUE (no log content is refused).  _merge adds counts and sums and takes the maximum;
 * _format_csv writes the trace's line shapes — "label,series,sector,t_ms,count" for every non-zero (bin, sector), "label,series,all,t_ms,count" for every
 * non-zero bin — plus "label,arrivals,all,overflow,count" and "label,done,all,overflow,count" where the overflows are non-zero; returns the text's length
 * (written in full only if it fits cap, then 0-terminated). */
int prach_noma_timeline_accumulate_logs(const prach_noma_timeline_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE,
                                        prach_noma_timeline *t, uint64_t *const series[6]);
void prach_noma_timeline_merge(const prach_noma_timeline_spec *, prach_noma_timeline *into, uint64_t *const into_series[6], const prach_noma_timeline *from,
                               const uint64_t *const from_series[6]);
size_t prach_noma_timeline_format_csv(const prach_noma_timeline_spec *, const prach_noma_timeline *, const uint64_t *const series[6], const char *label, char *buf,
                                      size_t cap);
int prach_noma_timeline_tile_ues(void);    /* UEs of one trial that one workgroup of prach::noma_timeline_kernel reduces (tests place sizes around it) */
int prach_noma_timeline_window_bins(void); /* bins of the LDS window of prach::noma_timeline_kernel (timeline_scheme 1), anchored at a tile's first arrival bin */

/* NOMA_C's NEAR-FAR PROFILE: per trial group, SECTOR and CHANNEL-GAIN LEVEL, what became of the UEs — the NOMA timeline with the arrival-bin axis replaced by
 * a gain-level axis.  The Rayleigh channel gain a UE draws at activation (NOMA.c:185-189) is the one quantity the pairing rests on (10*log(high) - 10*log(low)
 * against 15.0, NOMA.c:276) and it is not a field of THE NOMA MENU (the menu's field count is fixed); it is the axis of this kind instead.
 * THE GAIN LEVEL of a UE is L = prach_noma_gain_level(lgain), lgain = ln(gain) as prach_noma_activation_table gives it: L = floor(1000.0 * lgain), the product
 * ONE IEEE double multiplication, the floor towards minus infinity — the gain in hundredths of NOMA.c's own pairing unit 10 ln g: two UEs can pair when their
 * levels are 1500 apart.  The activation loop keeps gain >= 1e-7, so the levels of a trial lie in about -16 119 ... -3 350.  INT32_MIN is NO LEVEL: a
 * non-finite lgain, or |1000 lgain| >= 2^30.
 * THE DEFINITION is prach_noma_gain_accumulate_levels.  Class, SECTOR, SOJOURN, LOST and PTC are THE NOMA MENU's as they stand.  For UE i with level L:
 *   - every UE counts in its class counter (idle, served, dropped, pending): their sum is `ues`; an idle UE counts in nothing else;
 *   - an arrived UE is UNDEFINED FOR THE PROFILE if its SECTOR lies outside 0..5, if L is INT32_MIN, or if it is served and any of SOJOURN, LOST, PTC is negative
 *     (the menu's ONE RULE).  It counts in `undefined` and in nothing else below;
 *   - every other arrived UE counts in `defined` and in level_max / neg_level_max, and: L < lo: below += 1; L >= lo + bins * width (formed in 64 bits):
 *     above += 1; otherwise b = (L - lo) / width and arrived[s][b] += 1;
 *   - dropped and in a bin: dropped[s][b] += 1;
 *   - served: the scalars sojourn_sum += SOJOURN, lost_sum += LOST, ptc_sum += PTC, restarted += LOST > 0, always; in a bin: served[s][b] += 1 and the three
 *     sums at [s][b].
 * Pending per (sector, bin) is arrived - served - dropped; it is not stored.  IDENTITY: sum(arrived) + below + above + undefined == served + dropped + pending.
 * Under PRACH_FLAG_NOMA_NONSECTOR the sector is the UE's own, as in the timeline.  The six series are [ngroups][6 sectors][bins] each, in the order arrived,
 * served, dropped, sojourn_sum, lost_sum, ptc_sum.  Integers only, 64-bit outputs: device, host, forked workers and ranks merge exactly in any order. */
#define PRACH_NOMA_GAIN_SERIES 6
#define PRACH_NOMA_GAIN_MAX_BINS 4096
#define PRACH_NOMA_GAIN_NO_LEVEL INT32_MIN
typedef struct prach_noma_gain_spec {
    int32_t bins;      /* 1 .. PRACH_NOMA_GAIN_MAX_BINS */
    int32_t width;     /* >= 1, in level units */
    int32_t lo;        /* the level of the lower edge of bin 0: any int32 */
    int32_t ngroups;   /* number of output profiles */
    int32_t reserved;  /* 0 */
} prach_noma_gain_spec;

typedef struct prach_noma_gain { /* one per group */
    uint64_t trials;             /* trials accumulated (status PRACH_OK) */
    uint64_t ues;                /* sum of their nUE */
    uint64_t idle, served, dropped, pending; /* the four classes: idle + served + dropped + pending == ues */
    uint64_t undefined;          /* arrived UEs that are undefined for the profile (in no series, no sum, not below, not above) */
    uint64_t below, above;       /* defined arrived UEs with a level under bin 0 / at or above lo + bins * width */
    uint64_t restarted;          /* served, defined, LOST > 0 */
    uint64_t sojourn_sum, lost_sum, ptc_sum; /* over the defined served UEs, unbinned */
    uint64_t defined;            /* arrived UEs that are defined (each has a level): sum(arrived) + below + above; guards the two maxima */
    int64_t  level_max;          /* the largest level of a defined arrived UE; -1 where `defined` is 0 (a level may be -1: ask `defined`) */
    int64_t  neg_level_max;      /* the largest -L, i.e. minus the smallest level; -1 where `defined` is 0 */
} prach_noma_gain;

int32_t prach_noma_gain_level(double lgain);
/* the levels of every UE of a NOMA_C Philox cfg from prach_noma_activation_table (the host's libm): level[nUE].  PRACH_ERR_UNSUPPORTED: not NOMA_C, or
 * PRACH_RNG_GLIBC (the gain exists only inside the launch) */
int prach_noma_gain_levels(const prach_cfg *cfg, int32_t *level);
/* prach_run_trials plus the profiles, with the contract of prach_run_trials_noma_timeline word for word (groups, OVERWRITTEN outputs, a rerun trial counted
 * once, at most one reduction per call; results and logs are those of the same prach_run_trials call); g[ngroups] and series[q][ngroups * 6 * bins] are
 * caller-owned.  A pre-pass writes every UE's level from the launch's activation table on the device; the few UEs whose 1000 ln g lies within the error band
 * of an integer are resolved by the host (prach_timing.noma_gain_host_ues), so the result equals prach_noma_gain_accumulate_logs integer for integer whichever
 * side built the table; then prach::noma_gain_kernel (csrc/prach_noma_gain.hip) reduces.  Engine option "timeline_scheme" applies.
 * PRACH_ERR_ARG: a NULL output, bins or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED, before anything is launched: any cfg that is not NOMA_C; any NOMA_C cfg with rng_mode == PRACH_RNG_GLIBC; 36 * ngroups * bins > 2^27
 * words.  A refusal writes nothing. */
int prach_run_trials_noma_gain(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                               const prach_noma_gain_spec *spec, const int32_t *group, prach_noma_gain *g, uint64_t *const series[6]);
/* host side (no device needed), ONE group (series[q]: [6][bins]).  _accumulate_levels ADDS one trial's per-UE log with the levels AS GIVEN (any RNG mode:
 * THE DEFINITION); _accumulate_logs takes the levels from prach_noma_gain_levels(cfg) and calls it (PRACH_ERR_UNSUPPORTED: a cfg that is not NOMA_C or is
 * PRACH_RNG_GLIBC).  steps is the trial's prach_result.steps.  PRACH_ERR_ARG: a bad spec or cfg, a NULL pointer, nUE != cfg->nUE.  _merge adds counts and sums
 * and takes the maxima; _format_csv writes "label,series,sector,level,count" for every non-zero cell (level: the bin's lower edge lo + b * width),
 * "label,series,all,level,count" for every non-zero bin, and "label,arrived,all,below,count" / "label,arrived,all,above,count" where non-zero; returns the
 * text's length (written in full only if it fits cap, then 0-terminated). */
int prach_noma_gain_accumulate_levels(const prach_noma_gain_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, const int32_t *level,
                                      prach_noma_gain *g, uint64_t *const series[6]);
int prach_noma_gain_accumulate_logs(const prach_noma_gain_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_noma_gain *g,
                                    uint64_t *const series[6]);
void prach_noma_gain_merge(const prach_noma_gain_spec *, prach_noma_gain *into, uint64_t *const into_series[6], const prach_noma_gain *from,
                           const uint64_t *const from_series[6]);
size_t prach_noma_gain_format_csv(const prach_noma_gain_spec *, const prach_noma_gain *, const uint64_t *const series[6], const char *label, char *buf, size_t cap);
int prach_noma_gain_tile_ues(void);      /* UEs of one trial that one workgroup of prach::noma_gain_kernel reduces (tests place sizes around it) */
int prach_noma_gain_lds_max_bins(void);  /* the most bins whose counters the kernel keeps in LDS (timeline_scheme 1); more bins go straight to the global counters */

/* Per-trial summaries of NOMA_C trials: ONE ROW PER TRIAL — the four class counts, and for up to four NAMED fields of THE NOMA MENU above, over the UEs of
 * the classes in `who` whose value of the field is DEFINED (the menu's ONE RULE: >= 0), their number, sum, maximum and EXACT order statistics — selected on the
 * device, so that the spread between the seeds of a sweep point can be stated (prach_noma_summary_stats); the census pools the seeds into shared cells and
 * cannot.  NOMA's interesting quantities are spread over the classes (SOJOURN, TIMER, LOST and PTC of the served, AGE of the pending, RETX and MSG3FAIL of
 * the arrived), so the spec names them.
 * THE DEFINITION of a level is the summary's, taken per field: field x over its n[x] defined values in ONE trial at level m (permille) has rank
 * r = max(1, (n[x] * m + 999) / 1000), in 64-bit integers; the value is the r-th smallest.  No bins, no interpolation.
 * A defined value above prach_summary_max_value() (65 535) is a RANGE ERROR: it enters n, sum and max and no histogram; the levels of that field are -1 then
 * and the call returns PRACH_ERR_INTERNAL, as for the summary.  No trial produces one (csrc/prach_noma_menu.h, csrc/prach_noma_select.hip state the bounds).
 * `restarted` is counted over the SERVED UEs regardless of `who`: those whose LOST is defined and > 0. */
#define PRACH_NOMA_SUMMARY_MAX_FIELDS 4
typedef struct prach_noma_summary_spec {
    int32_t who;                 /* PRACH_NOMA_* class bits, not 0 */
    int32_t nfields;             /* 1 .. 4; the fields behind it must be 0 */
    int32_t field[PRACH_NOMA_SUMMARY_MAX_FIELDS];   /* PRACH_NOMA_* ids; ONE is allowed (its levels are 0); a field may be named twice */
    int32_t nq;                  /* 1 .. PRACH_SUMMARY_MAX_Q */
    int32_t permille[PRACH_SUMMARY_MAX_Q];          /* 1 .. 1000; the levels behind nq are ignored, as in prach_summary_spec */
    int32_t reserved[2];         /* 0 */
} prach_noma_summary_spec;
typedef struct prach_noma_trial_summary {   /* one per TRIAL */
    int32_t status, nUE;
    int32_t idle, served, dropped, pending;  /* counted regardless of `who`; their sum is nUE */
    int32_t selected;                        /* class in `who` */
    int32_t restarted;                       /* served UEs with LOST defined and > 0, regardless of `who` */
    int32_t range_errors, reserved;
    int32_t n[PRACH_NOMA_SUMMARY_MAX_FIELDS];    /* selected UEs whose value of field x is DEFINED */
    int64_t sum[PRACH_NOMA_SUMMARY_MAX_FIELDS];  /* over those */
    int32_t max[PRACH_NOMA_SUMMARY_MAX_FIELDS];  /* -1 if n[x] == 0 */
    int32_t q[PRACH_NOMA_SUMMARY_MAX_FIELDS][PRACH_SUMMARY_MAX_Q]; /* -1 if n[x] == 0, level unused or field unused */
} prach_noma_trial_summary;

/* prach_run_trials plus one NOMA summary row per trial; the row contract is prach_run_trials_summary's: rows[n] is caller-owned and OVERWRITTEN; a trial that
 * is not PRACH_OK carries its status and nUE, zeros, and -1 in every maximum and level; a trial the engine reruns — a split call, the resolver's ambiguity
 * rerun — is written once, by the launch whose result is kept.  prach::noma_summary_kernel (csrc/prach_noma_select.hip) selects from the log records
 * prach::noma_kernel writes ON THE DEVICE, one workgroup per trial.
 * PRACH_ERR_ARG: a NULL spec or output; an unknown field or class bit, an empty `who`; nfields, nq or a level out of range; a non-zero unused field or
 * reserved word;
 * PRACH_ERR_UNSUPPORTED, before anything is launched: any cfg that is not NOMA_C; any NOMA_C cfg with rng_mode == PRACH_RNG_GLIBC.  PRACH_FLAG_NOMA_NONSECTOR
 * is accepted. */
int prach_run_trials_noma_summary(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                  const prach_noma_summary_spec *spec, prach_noma_trial_summary *rows);
/* NOMA summaries, host side (no device needed; both RNG modes).
 * prach_noma_summary_from_logs OVERWRITES *row with the summary of one trial's per-UE log: THE DEFINITION prach::noma_summary_kernel equals, integer for
 * integer (it sorts, so any int32 value is handled and range_errors is 0; status PRACH_OK).  steps is the trial's prach_result.steps.
 * PRACH_ERR_UNSUPPORTED: a cfg that is not NOMA_C.  PRACH_ERR_ARG: a bad spec or cfg, a NULL pointer, nUE != cfg->nUE (no log content is refused). */
int prach_noma_summary_from_logs(const prach_noma_summary_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE,
                                 prach_noma_trial_summary *row);
/* Mean and spread over the trials of each group, with prach_summary_stats' rules (groups, two passes in trial order, in doubles, sd and sem, n = 0 and 1):
 * out[ngroups][4 + nfields * (1 + nq)], the metrics in this order:
 *   served_ratio (served / nUE), dropped_ratio (dropped / nUE), pending_ratio (pending / nUE), restart_ratio (restarted / served),
 *   then per field x, in the spec's order: <name>_mean (sum[x] / n[x]) and <name>_p<m> for every level, <name> the field's name in lower case.
 * A row whose status is not PRACH_OK is skipped for every metric; a row with nUE == 0 for the three class ratios, one with served == 0 for restart_ratio, one
 * with n[x] == 0 for field x's metrics.  PRACH_ERR_ARG: a bad spec, a NULL argument, a group id out of range. */
int prach_noma_summary_stats(const prach_noma_summary_spec *, const prach_noma_trial_summary *rows, int n, const int32_t *group, int ngroups, prach_stat *out);
/* one group (4 + nfields * (1 + nq) prach_stat) as text, in prach_summary_format_csv's line format */
size_t prach_noma_summary_format_csv(const prach_noma_summary_spec *, const prach_stat *stats_of_one_group, const char *label, char *buf, size_t cap);

/* Pick per trial of NOMA_C trials, selected on the device: WHICH UEs stand behind a count of the census — the contract of prach_run_trials_pick word for word
 * (selected, matched and undefined; the three orders; stored = min(matched, k), threshold and ties_left_out; OVERWRITTEN outputs, zero rows behind `stored`, a
 * rerun trial written once; keys RANKED in 0 .. prach_summary_max_value(), range_errors voiding the trial's rows and failing the call with
 * PRACH_ERR_INTERNAL), with a prach_pick_spec whose `who` is PRACH_NOMA_* class bits (all four) and whose clause fields and key field are PRACH_NOMA_* ids, the
 * values those of THE NOMA MENU above with its ONE RULE.  The header is prach_pick, a row the 80-byte prach_pick_row: the log record as logged, a(i) (-1 for an
 * IDLE UE) and the key.  No trial produces a key outside the ranked range: ARRIVAL, COMPLETION and AGE are subframe numbers of a trial of 10 000 + 6 subframes,
 * SOJOURN and LOST at most that, STATE at most 8, SECTOR at most 5, MSG3FAIL the upper half of a word; TIMER, PTC, RETX and PREAMBLE are logged words that
 * grow by at most one per subframe or name one of at most 64 preambles (csrc/prach_noma_select.hip restates the bounds).
 * prach::noma_pick_kernel (csrc/prach_noma_select.hip) selects from the log records prach::noma_kernel writes ON THE DEVICE, one workgroup per trial, and
 * leaves a trial's rows in UE-index order; the engine sorts the at most k rows of a trial into the defined order on the host.
 * PRACH_ERR_ARG: the argument cases of prach_run_trials_pick, with NOMA's ids and bits;
 * PRACH_ERR_UNSUPPORTED, before anything is launched: any cfg that is not NOMA_C; any NOMA_C cfg with rng_mode == PRACH_RNG_GLIBC; n * k * 10 + n * 8 > 2^27
 * words.  PRACH_FLAG_NOMA_NONSECTOR is accepted. */
int prach_run_trials_noma_pick(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_pick_spec *spec,
                               prach_pick *picks, prach_pick_row *rows);
/* THE DEFINITION prach::noma_pick_kernel plus the engine's sort equal, integer for integer (no device needed; both RNG modes): the pick of ONE trial from its
 * per-UE log; steps is the trial's prach_result.steps.  It lists and sorts, so any int32 key is handled and its range_errors is 0.  PRACH_ERR_ARG: a bad spec
 * or cfg, a NULL pointer, nUE != cfg->nUE; PRACH_ERR_UNSUPPORTED: a cfg that is not NOMA_C.  _format_csv writes prach_pick_format_csv's lines. */
int prach_noma_pick_from_logs(const prach_pick_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_pick *hdr, prach_pick_row *rows);
size_t prach_noma_pick_format_csv(const prach_pick_spec *, const prach_pick *, const prach_pick_row *rows, const char *label, int trial, uint64_t seed, char *buf,
                                  size_t cap);

/* Per-subframe preamble trace per trial group, recorded by the simulation kernels WHILE THEY RUN and reduced on the device: how many preambles were used,
 * decoded and collided in each stretch of the simulation — the quantities TR 37.868's collision probability is defined on.  Unlike the four reductions above
 * this is not a function of the per-UE state a trial leaves behind (prach_result has only the two whole-trial totals collisionPreambles and
 * totalPreambleTxop), so there is no prach_trace_accumulate_logs: the logs do not hold it.  Per subframe t of a trial, in the reference's own terms:
 *   calls       preambleCollision invocations (Beta.c:315 / WithNOMA:607): one per preamble that at least one matched UE transmits = preambles USED
 *   singles     the calls with check == 1 = preambles DECODED; calls - singles = preambles COLLIDED.  These three mean the same in both programs
 *   txop        what the subframe added to totalPreambleTxop   } as the programs count them, and they weight them differently: Beta.c adds 1 per call and 1
 *   collisions  what the subframe added to collisionPreambles  } per collided call (Beta.c:334,349-351: txop = calls, collisions = calls - singles);
 *               RandomAccessWithNOMA.c adds 1 per single and `check`, the number of UEs on the preamble, per collided call to both (WithNOMA:650-652)
 * A trial's rows cover the subframes [0, steps); a subframe in which nothing was resolved is all zero.  Bin b covers [b * bin_ms, (b + 1) * bin_ms).  A
 * subframe at or behind bins * bin_ms counts in the scalars and in no bin; its calls are in overflow_calls.  Summed over a trial, txop and collisions are
 * the trial's prach_result.totalPreambleTxop and collisionPreambles.  Integers only: device, host, forked workers and ranks merge exactly in any order.
 * Beta.c and RandomAccessWithNOMA.c only, in both RNG modes: NOMA.c's resolver is another one (a NOMA_C cfg is PRACH_ERR_UNSUPPORTED, before anything is
 * launched).  A trace call runs the kernels engine option "fast" = 0 selects (prach::lcluster_kernel records nothing); results, logs and the other timing
 * fields are those of the same prach_run_trials call. */
#define PRACH_TRACE_MAX_BINS 65536         /* Uniform traffic at 1 ms: 60 000 bins */

typedef struct prach_trace_spec {
    int32_t bins;      /* 1 .. PRACH_TRACE_MAX_BINS */
    int32_t bin_ms;    /* >= 1 */
    int32_t ngroups;   /* number of output traces */
    int32_t reserved;  /* 0 */
} prach_trace_spec;

typedef struct prach_trace {         /* one per group */
    uint64_t trials;                 /* trials accumulated (status PRACH_OK) */
    uint64_t subframes;              /* sum of their steps */
    uint64_t calls, singles, txop, collisions; /* over all their subframes, unbinned */
    uint64_t overflow_calls;         /* calls in subframes at or behind bins * bin_ms (in no bin) */
    int64_t  calls_max;              /* the largest `calls` of one subframe of one trial; -1 without subframes */
} prach_trace;

/* prach_run_trials plus the traces, with the contract of prach_run_trials_timeline: trial k is added to group group[k] (group == NULL: trial k is group k and
 * ngroups must equal n); tr[ngroups] and the four series [ngroups * bins] are caller-owned and OVERWRITTEN; a trial whose final status is not PRACH_OK
 * contributes nothing; a trial the engine reruns contributes once, from the launch whose result is kept.  The simulation kernels write one 16-byte row per
 * subframe ON THE DEVICE (the arena of the call grows by 16 bytes x maxTime per trial) and prach::trace_kernel (csrc/prach_trace.hip) reduces them there.
 * PRACH_ERR_ARG: a NULL output, a bin count or width out of range, a group id out of range, NULL group with ngroups != n;
 * PRACH_ERR_UNSUPPORTED: any NOMA_C cfg; 4 * ngroups * bins > 2^27 words (1 GiB of device buffer). */
int prach_run_trials_trace(prach_engine *, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                           const prach_trace_spec *spec, const int32_t *group, prach_trace *tr, uint64_t *calls, uint64_t *singles, uint64_t *txop,
                           uint64_t *collisions);

/* engine tunables; none changes a result, all are covered by parity tests:
 *   "cluster"       workgroups cooperating on one trial (1..64; 0 = auto)
 *   "stream_factor" glibc mode: initial draws-per-UE budget of the rand() stream window (0 = auto; it grows on demand)
 *   "legacy"        1: run on the one-workgroup-per-trial kernel (the exact fallback of every capacity check)
 *   "dense"         1: cluster kernel without the compacted two-phase pass
 *   "wide_records"  1: 16-byte hot records also with one workgroup per trial
 *   "pipeline"      0: a cluster does not run phase A of the next subframe during the exchange of the current one
 *   "resident"      test hook: treat only this many workgroups as co-resident (0 = ask the runtime's occupancy query)
 *   "host_threads"  NOMA_C: host threads that build the activation tables (0 = all cores)
 *   "lds_records"   0: clusters keep their UE records in global memory instead of LDS
 *   "fast"          0: LDS-resident clusters run on the general cluster kernel instead of prach::lcluster_kernel
 *   "batch"         0: one-workgroup-per-trial Philox launches run on the general cluster kernel instead of prach::batch_kernel
 *   "xcd_pack"      0: clusters are not launched XCD-packed
 *   "batch_waves"   prach::batch_kernel's workgroup shape: 8 (512 threads, two trials per CU), 16 (1024 threads), 0 = chosen per launch
 *   "plain_arena"   1: the device arena is one hipMalloc allocation, re-allocated when it grows (before the first call only; diagnostic)
 *   "mem_budget_mb" arena megabytes one launch may take (default: three quarters of the device's memory): a call that needs more runs as several launches
 *   "dist_scheme"   prach::dist_kernel's binning of the preamble counts: 0 one LDS atomic per UE, 1 the same into per-wavefront copies of the 256 bins
 *                   (the default: measured fastest), 2 one LDS atomic per distinct value of a wavefront (match and aggregate)
 *   "timeline_scheme" prach::timeline_kernel's binning: 0 every contribution is a 64-bit global atomic, 1 windows of bins privatised in LDS per workgroup
 *                   (the default: measured 15-20x faster on the sweep grids)
 *   "sojourn_scheme" prach::sojourn_kernel's binning: 0 every contribution is a 64-bit agent-scope global atomic, 1 rows of the histogram privatised in LDS
 *                   per workgroup (the default: measured 95x faster on the sweep grids)
 *   "xtab_scheme"   prach::xtab_kernel's binning: 0 every contribution is a 64-bit agent-scope global atomic, 1 a table of at most
 *                   prach_xtab_window_words() cells privatised in LDS per workgroup, a larger one as under 0 (the default)
 *   "trace_scheme"  prach::trace_kernel's binning: 0 every contribution is a 64-bit agent-scope global atomic, 1 a tile's bins added up in an LDS window first
 *                   (the default)
 *   "summary_threads" prach::summary_kernel's workgroup: 512 or 1024 threads (0 = the default, 1024)
 *   "pick_threads"  prach::pick_kernel's workgroup: 512 or 1024 threads (0 = the default, 1024)
 *   "calendar_cap", "vmm_fail_after", "noma_ambiguity_test", "noma_host_activation"   test hooks (prach_engine.hip) */
int prach_engine_set(prach_engine *, const char *key, int64_t value);

/* Host-side pieces of the same seam (no device needed) */
void prach_cfg_defaults(prach_cfg *cfg, int variant); /* Beta.c:47-57 / WithNOMA:70-88 */
int prach_cfg_validate(const prach_cfg *cfg);
int prach_max_time(const prach_cfg *cfg);
/* What this trial costs inside a batched launch, in kernel microseconds on an MI355X (a measured table, prach_host.c): the weight the multi-GPU dealing of the
   --times x sweep grid balances — the reference runs that grid serially (RandomAccessWithNOMA.c:216-221), so there is nothing there to replace. */
double prach_trial_cost(const prach_cfg *cfg);
/* out[s] = activeCheck after the arrival update of access slot s (Beta.c:121-134); returns #slots */
int prach_arrival_schedule(const prach_cfg *cfg, int32_t *out, int cap, int32_t *nAccessUE);
/* k-th .. k+n-th values of srand(seed)/rand() */
void prach_glibc_stream(uint32_t seed, uint64_t first, uint64_t n, int32_t *out);
/* the same stream generated ON THE DEVICE (what glibc-mode trials consume): the host jumps ahead with 31x31 matrix
 * powers of the lagged-Fibonacci recurrence, one wavefront per 63 488-value chunk rolls it forward */
int prach_device_glibc_stream(prach_engine *, uint32_t seed, uint64_t first, uint64_t n, int32_t *out);
const char *prach_strerror(int status);

/* NOMA.c variant (PRACH_VARIANT_NOMA_C): per-UE attributes fixed at activation (activeUE, NOMA.c:131-192):
 * first preamble, sector, Rayleigh channel gain and its natural log (the pairing test of NOMA.c:276 uses
 * 10*log(high)-10*log(low)), and the number of draws the activation consumed.  This is the HOST form, with the libm the
 * reference links (cos, sin, log, pow).  The engine builds the table on the DEVICE (prach_noma_activation_table_device below is that
 * kernel on its own) and calls the host form only for the UEs the kernel flags: wherever a last-bits difference between the device's
 * math library and the host's could change a float rounding, the rejection test or the draw count.  Engine option
 * "noma_host_activation" = 1 builds the whole table with the functions here instead (the round-1/2 behaviour).
 * This table form is the Philox mode's (draw k of UE i is independent of every other UE).  In glibc mode the rejection loops make
 * every stream position data dependent: there the whole trial is one launch with activeUE inside it (same error bands); a trial that hits
 * a band is run again slot by slot, its arrivals activated one by one with prach_noma_activation_stream below. */
int prach_noma_activation_table(const prach_cfg *cfg, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                uint32_t *ndraws);
/* the same for the UEs [lo, hi) only (outputs indexed from lo): ranges are independent, the engine builds them on all host cores */
int prach_noma_activation_range(const prach_cfg *cfg, int lo, int hi, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                uint32_t *ndraws);
/* The device-built table as the engine uses it (Philox mode), copied back: preamble0 / sector / ndraws of every UE equal the host form's;
 * gain / lgain of an unflagged UE are within a few ulp of it (never read except through comparisons that carry an error band), those of a
 * flagged UE (flagged[i] != 0; nullable) are the host form's, recomputed by this call.  For tests and diagnosis. */
int prach_noma_activation_table_device(prach_engine *, const prach_cfg *cfg, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                       uint32_t *ndraws, uint8_t *flagged);
/* activeUE for ONE UE in the reference's own rand() stream (glibc mode of the NOMA_C variant): draws stream[*pos...] in the reference's
 * order, *pos advances; PRACH_ERR_STREAM when the window of `avail` values is exhausted */
int prach_noma_activation_stream(const prach_cfg *cfg, const int32_t *stream, uint64_t *pos, uint64_t avail, int32_t *preamble0, int32_t *sector,
                                 double *gain, double *lgain);
size_t prach_format_noma_line(const prach_cfg *, const prach_result *, char *buf, size_t cap); /* NOMA.c:606-632 */

/* Distributions, host side (no device needed).  d / delay_hist / ptc_hist: ONE group (delay_bins and PRACH_DIST_PTC_BINS entries).
 * prach_dist_accumulate_logs ADDS one trial's per-UE log to a group: the definition prach::dist_kernel equals, integer for integer
 * (PRACH_ERR_ARG: a bad spec, or a successful UE with a negative timer — nothing has been added then). */
int prach_dist_accumulate_logs(const prach_dist_spec *, const prach_ue_log *ue, int nUE, prach_dist *d, uint64_t *delay_hist, uint64_t *ptc_hist);
/* counts are summed, delay_max is the maximum */
void prach_dist_merge(const prach_dist_spec *, prach_dist *into, uint64_t *dh_into, uint64_t *ph_into, const prach_dist *from, const uint64_t *dh_from,
                      const uint64_t *ph_from);
/* lower edge (ms) of the first delay bin whose cumulative count reaches max(1, ceil(q * success)); -1 if success == 0 or that rank lies in the overflow */
int64_t prach_dist_delay_quantile(const prach_dist_spec *, const prach_dist *, const uint64_t *delay_hist, double q);
/* one group as text: `label,delay,<lower edge ms>,<count>,<cumulative share %.6f>` per non-empty delay bin, `label,delay,overflow,<count>,1.000000` if the
 * overflow is non-zero, then `label,ptx,<k>,<count>,<cumulative share>` per non-empty preamble-count bin; lines end in \n.  Returns the length needed
 * (without the terminating 0); the text is written only if it fits cap with its terminator. */
size_t prach_dist_format_csv(const prach_dist_spec *, const prach_dist *, const uint64_t *delay_hist, const uint64_t *ptc_hist, const char *label, char *buf,
                             size_t cap);
int prach_dist_tile_ues(void); /* UEs of one trial that one workgroup of prach::dist_kernel reduces (tests place sizes around it) */

/* Timelines, host side (no device needed).  t and the five series: ONE group (`bins` entries each).
 * prach_timeline_accumulate_logs ADDS one trial's per-UE log to a group: THE DEFINITION prach::timeline_kernel equals, integer for integer.
 * PRACH_ERR_UNSUPPORTED: a NOMA_C cfg.  PRACH_ERR_ARG: a bad spec or cfg, nUE != cfg->nUE, or a successful UE with a negative timer or with
 * c(i) < a(i) (nothing has been added then). */
int prach_timeline_accumulate_logs(const prach_timeline_spec *, const prach_cfg *cfg, const prach_ue_log *ue, int nUE, prach_timeline *t, uint64_t *arrivals,
                                   uint64_t *success, uint64_t *sojourn_sum, uint64_t *timer_sum, uint64_t *done);
/* counts and sums are added, done_max is the maximum.  The series arguments are, for `into` and then for `from`: arrivals, success, sojourn_sum, timer_sum, done */
void prach_timeline_merge(const prach_timeline_spec *, prach_timeline *into, uint64_t *const into_series[5], const prach_timeline *from,
                          const uint64_t *const from_series[5]);
/* one group as text: `label,<series>,<lower edge ms>,<value>` per non-zero bin, series by series (arrivals, success, sojourn_sum, timer_sum, done), with
 * `label,arrivals,overflow,<count>` behind the arrivals and `label,done,overflow,<count>` behind the done lines where the counter is non-zero; lines end in \n.
 * Returns the length needed (without the terminating 0); the text is written only if it fits cap with its terminator. */
size_t prach_timeline_format_csv(const prach_timeline_spec *, const prach_timeline *, const uint64_t *const series[5], const char *label, char *buf, size_t cap);
int prach_timeline_tile_ues(void);    /* UEs of one trial that one workgroup of prach::timeline_kernel reduces (tests place sizes around it) */
int prach_timeline_window_bins(void); /* bins of the LDS windows of prach::timeline_kernel (timeline_scheme 1), anchored at a tile's first arrival bin */

/* Sojourn histograms, host side (no device needed).  j, hist [arrival_bins][delay_bins], row_arrived and row_delay_overflow [arrival_bins]: ONE group.
 * prach_sojourn_accumulate_logs ADDS one trial's per-UE log to a group: THE DEFINITION prach::sojourn_kernel equals, integer for integer.  Errors as
 * prach_timeline_accumulate_logs: PRACH_ERR_UNSUPPORTED: a NOMA_C cfg.  PRACH_ERR_ARG: a bad spec or cfg, nUE != cfg->nUE, or a successful UE with a negative
 * timer or with c(i) < a(i) (nothing has been added then). */
int prach_sojourn_accumulate_logs(const prach_sojourn_spec *, const prach_cfg *cfg, const prach_ue_log *ue, int nUE, prach_sojourn *j, uint64_t *hist,
                                  uint64_t *row_arrived, uint64_t *row_delay_overflow);
/* counts and sums are added, sojourn_max is the maximum */
void prach_sojourn_merge(const prach_sojourn_spec *, prach_sojourn *into, uint64_t *hist_into, uint64_t *arrived_into, uint64_t *overflow_into,
                         const prach_sojourn *from, const uint64_t *hist_from, const uint64_t *arrived_from, const uint64_t *overflow_from);
/* the rule of prach_dist_delay_quantile on one arrival row, or pooled over all rows (row == -1): the lower edge (ms) of the first delay bin whose cumulative
 * count reaches max(1, ceil(q * n)), n = the row's successful UEs including its overflow; -1 if n == 0, that rank lies in the overflow, or an argument is bad */
int64_t prach_sojourn_quantile(const prach_sojourn_spec *, const uint64_t *hist, const uint64_t *row_delay_overflow, int row, double q);
/* one group as text, row by row: `label,<row lower edge ms>,arrived,<count>` where the row has arrivals, `label,<row lower edge ms>,<delay lower edge ms>,<count>`
 * per non-zero cell, `label,<row lower edge ms>,overflow,<count>` where the row's overflow is non-zero; behind the rows `label,arrivals,overflow,<count>` where
 * arrival_overflow is non-zero; lines end in \n.  Returns the length needed (without the terminating 0); the text is written only if it fits cap with its
 * terminator. */
size_t prach_sojourn_format_csv(const prach_sojourn_spec *, const prach_sojourn *, const uint64_t *hist, const uint64_t *row_arrived,
                                const uint64_t *row_delay_overflow, const char *label, char *buf, size_t cap);
int prach_sojourn_tile_ues(void);     /* UEs of one trial that one workgroup of prach::sojourn_kernel reduces (tests place sizes around it) */
int prach_sojourn_window_words(void); /* 32-bit cells of the LDS window of prach::sojourn_kernel (sojourn_scheme 1): it holds window_words / delay_bins rows */

/* Cross-tabulation, host side (no device needed).  xt and cells [row_bins + 1][col_bins + 1]: ONE group.
 * prach_xtab_accumulate_logs ADDS one trial's per-UE log to a group: THE DEFINITION prach::xtab_kernel equals, integer for integer.  steps is the trial's
 * prach_result.steps.  PRACH_ERR_UNSUPPORTED: a NOMA_C cfg.  PRACH_ERR_ARG: a bad spec or cfg, nUE != cfg->nUE (no log content is refused: a bad value is
 * UNDEFINED). */
int prach_xtab_accumulate_logs(const prach_xtab_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_xtab *xt, uint64_t *cells);
/* counts and sums are added, row_max and col_max are the maxima */
void prach_xtab_merge(const prach_xtab_spec *, prach_xtab *into, uint64_t *cells_into, const prach_xtab *from, const uint64_t *cells_from);
/* the rule of prach_sojourn_quantile along the column axis of one row (0 .. row_bins, the overflow row included), or pooled over all rows (row == -1): the
 * lower edge of the first regular column bin whose cumulative count reaches max(1, ceil(q * n)), n = the row's UEs including its overflow column; -1 if
 * n == 0, that rank lies in the overflow column, or an argument is bad */
int64_t prach_xtab_quantile(const prach_xtab_spec *, const uint64_t *cells, int row, double q);
/* one group as text: `label,<row lower edge>,<column lower edge>,<count>` per non-zero cell in row-major order, an overflow bin's edge spelled `overflow`;
 * behind them `label,undefined,,<count>` where undefined is non-zero; lines end in \n.  Returns the length needed (without the terminating 0); the text is
 * written only if it fits cap with its terminator. */
size_t prach_xtab_format_csv(const prach_xtab_spec *, const prach_xtab *, const uint64_t *cells, const char *label, char *buf, size_t cap);
int prach_xtab_tile_ues(void);     /* UEs of one trial that one workgroup of prach::xtab_kernel reduces (tests place sizes around it) */
int prach_xtab_window_words(void); /* the largest table, in cells, that prach::xtab_kernel privatises in LDS (xtab_scheme 1) */

/* Per-trial summaries, host side (no device needed).
 * prach_summary_from_logs OVERWRITES *row with the summary of one trial's per-UE log: THE DEFINITION prach::summary_kernel equals, integer for integer (it
 * sorts, so any int32 value is handled and range_errors is 0; status PRACH_OK).  Errors as prach_timeline_accumulate_logs. */
int prach_summary_from_logs(const prach_summary_spec *, const prach_cfg *cfg, const prach_ue_log *ue, int nUE, prach_trial_summary *row);
/* Mean and spread over the trials of each group: out[ngroups][5 + 3 * nq], the metrics in this order:
 *   success_ratio (success / nUE), restart_ratio (restarted / success), sojourn_mean, timer_mean, ptx_mean (sum / success),
 *   sojourn_p<m> for every level, timer_p<m> ..., ptx_p<m> ...
 * Trial k belongs to group group[k] (group == NULL: all trials are group 0 and ngroups must be 1).  A row whose status is not PRACH_OK is skipped for every
 * metric; a row with success == 0 is skipped for every metric but success_ratio.  Two passes in trial order, in doubles: mean = sum(x) / n,
 * sd = sqrt(sum((x - mean)^2) / (n - 1)), sem = sd / sqrt(n); sd = sem = 0 for n = 1, everything 0 for n = 0.  No t-quantiles: n is given, the reader picks
 * the interval.  PRACH_ERR_ARG: a bad spec, a NULL argument, a group id out of range. */
int prach_summary_stats(const prach_summary_spec *, const prach_trial_summary *rows, int n, const int32_t *group, int ngroups, prach_stat *out);
/* one group (5 + 3 * nq prach_stat) as text: `label,<metric>,<n>,<mean>,<sd>,<sem>,<min>,<max>` per metric, numbers as %.9g, lines end in \n.  Returns the
 * length needed (without the terminating 0); the text is written only if it fits cap with its terminator. */
size_t prach_summary_format_csv(const prach_summary_spec *, const prach_stat *stats_of_one_group, const char *label, char *buf, size_t cap);
int prach_summary_max_value(void);    /* 65 535: the largest value prach::summary_kernel ranks */

/* Picks, host side (no device needed).
 * prach_pick_from_logs OVERWRITES *hdr and rows[spec->k] with the pick of one trial's per-UE log: THE DEFINITION prach::pick_kernel and the engine's sort
 * equal, integer for integer, by filtering and sorting (it sorts, so any key is handled and range_errors is 0; status PRACH_OK).  steps is the trial's
 * prach_result.steps.  PRACH_ERR_UNSUPPORTED: a NOMA_C cfg.  PRACH_ERR_ARG: a bad spec or cfg, nUE != cfg->nUE (no log content is refused: a bad value is
 * UNDEFINED). */
int prach_pick_from_logs(const prach_pick_spec *, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_pick *hdr, prach_pick_row *rows);
/* one trial as text: the header line `label,<trial>,<seed>,<nUE>,header,<status>,<selected>,<matched>,<stored>,<undefined>,<threshold>,<ties_left_out>`, then
 * one line per stored row, `label,<trial>,<seed>,<nUE>,<rank from 0>,<key>,<arrival>,` and the 16 logged fields in the order of prach_ue_log; lines end in \n.
 * Returns the length needed (without the terminating 0); the text is written only if it fits cap with its terminator. */
size_t prach_pick_format_csv(const prach_pick_spec *, const prach_pick *hdr, const prach_pick_row *rows, const char *label, int trial, uint64_t seed, char *buf,
                             size_t cap);

/* Traces, host side (no device needed).  t and the four series (calls, singles, txop, collisions): ONE group (`bins` entries each).  There is no
 * prach_trace_accumulate_logs: a per-UE log does not hold what happened per subframe (the block above).
 * counts and sums are added, calls_max is the maximum */
void prach_trace_merge(const prach_trace_spec *, prach_trace *into, uint64_t *const into_series[4], const prach_trace *from, const uint64_t *const from_series[4]);
/* one group as text: `label,<series>,<lower edge ms>,<value>` per non-zero bin, series by series (calls, singles, txop, collisions), then
 * `label,calls,overflow,<count>` where overflow_calls is non-zero; lines end in \n.  Returns the length needed (without the terminating 0); the text is
 * written only if it fits cap with its terminator. */
size_t prach_trace_format_csv(const prach_trace_spec *, const prach_trace *, const uint64_t *const series[4], const char *label, char *buf, size_t cap);
int prach_trace_tile_subframes(void); /* subframes of one trial that one workgroup of prach::trace_kernel reduces (tests place sizes around it) */

/* Text surfaces, byte-compatible with the reference (latency values excepted) */
size_t prach_format_logs(const prach_ue_log *ue, int nUE, char *buf, size_t cap);           /* Beta.c:501 */
size_t prach_format_results(const prach_cfg *, const prach_result *, double latency_s, char *buf, size_t cap); /* Beta.c:460-482 / WithNOMA:762-793 */
size_t prach_format_stdout(const prach_cfg *, const prach_result *, double latency_s, char *buf, size_t cap);  /* Beta.c:200-206,440-446 / WithNOMA:354-361,741-748 */
int prach_result_file_name(const prach_cfg *, int is_log, char *buf, size_t cap);            /* Beta.c:452-456,490-494 / WithNOMA:754-758,801-805 */
int prach_write_trial_files(const prach_cfg *, const prach_result *, const prach_ue_log *ue, double latency_s,
                            const char *root_dir);

/* results.csv (AveragePerformance.py:7-24): per nUE point the six lines of every seed's Beta.c Results.txt
 * are summed in seed order (Python floats = doubles), divided by the number of seeds, rounded with
 * np.around(x, 3) and written by csv.writer (shortest float repr, CRLF line ends, no header).
 * prach_results_csv_accumulate adds one Results.txt text to acc[6]; prach_results_csv_row formats one row. */
int prach_results_csv_accumulate(double acc[6], const char *results_txt);
size_t prach_results_csv_row(const double acc[6], int nseeds, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
