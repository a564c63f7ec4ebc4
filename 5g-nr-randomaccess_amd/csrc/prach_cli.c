/* prach_cli.c — `prach_sim`: host-C driver with the reference's command-line surface
 * (RandomAccessWithNOMA.c:90-206, README.md:43-87) on top of the C ABI (include/prach.h).
 *
 * Same (flag, value) pair parsing, same messages and exit(-1) on bad values, same seed loop x
 * nUE sweep (WithNOMA:216-221), same stdout block and result files; the per-subframe loop itself
 * runs on the MI355X through prach_run_trials().  Both the spellings the code accepts (-rc, -mrc,
 * -bs, -ut) and the ones README.md documents (-r, -m, -u) are taken; `-d 2` selects Beta as the
 * README says (the reference's validation rejects it).
 *
 * `--program noma` runs NOMA.c's loop instead (NOMA.c:644-717: 10 seeds by default, one result line per
 * (seed, nUE) on stdout and appended to TestResults/Sector_{nUE}_Result.txt, "Done" per seed); that
 * variant draws from Philox by default; `--rng glibc` runs it in the reference's own rand() stream (prach_noma_glibc.hip: one launch per
 * sweep point, the seeds side by side), chained over the sweep of a seed like NOMA.c:644-647.
 *
 * Extensions (not in the reference): --program beta|withnoma|noma, --rng glibc|philox, --nue N,
 * --sweep LO:HI:STEP, --out DIR, --logs 0|1, --device N, --csv FILE (--program beta: the results.csv of
 * AveragePerformance.py over the --times seeds of every sweep point, written by prach_results_csv_*),
 * --sector-grants 1 (--program withnoma) / --nonsector 1 (--program noma): the two code paths the reference carries
 * commented out (WithNOMA:312,626-637 / NOMA.c:325-447,688);
 * --cdf FILE [--cdf-bins N] [--cdf-bin-ms W]: the distributions of access delay and of the number of preamble transmissions of the successful UEs
 * (prach_run_trials_dist: reduced on the device, so it works with --logs 0), one group per sweep point with the --times seeds merged, labelled nUE
 * (default 4096 bins of 1 ms);
 * --timeline FILE [--timeline-bin MS]: arrivals, successes, sojourn and timer sums by arrival time and completions by completion time
 * (prach_run_trials_timeline: reduced on the device, so it works with --logs 0), one group per sweep point with the --times seeds merged, labelled nUE;
 * bins of MS ms (default 5) that cover the whole horizon, maxTime + 6 ms; --program beta|withnoma only, and not together with --cdf (one reduction per call);
 * --sojourn FILE [--sojourn-arrival-ms MS] [--sojourn-bin MS]: the histogram of the time from arrival to Msg4 by arrival row (prach_run_trials_sojourn: reduced
 * on the device, so it works with --logs 0), one group per sweep point with the --times seeds merged, labelled nUE; rows of MS ms (default 500) over maxTime,
 * delay bins of MS ms (default 5) over maxTime + 6 ms; --program beta|withnoma only, and not together with --cdf or --timeline;
 * --ci FILE [--ci-levels M1,M2,...]: mean, standard deviation, standard error, minimum and maximum ACROSS THE --times SEEDS of every sweep point (labelled nUE)
 * of the success and restart ratio, the mean sojourn / timer / preamble transmissions and their exact per-trial percentiles at the given levels in permille
 * (default 500,950,990; at most 8): one row per trial comes from the device (prach_run_trials_summary, so it works with --logs 0), the statistics are
 * prach_summary_stats over the rows in trial order; --program beta|withnoma only, and not together with --cdf, --timeline or --sojourn;
 * --trace FILE [--trace-bin MS]: the per-subframe preamble trace — preambles used (calls), decoded (singles), and what the programs add to totalPreambleTxop
 * and collisionPreambles, by time (prach_run_trials_trace: recorded by the simulation kernels and reduced on the device, so it works with --logs 0), one group
 * per sweep point with the --times seeds merged, labelled nUE; bins of MS ms (default 5) that cover maxTime; --program beta|withnoma only, and not together
 * with --cdf, --timeline, --sojourn or --ci (one reduction per call);
 * --xtab FILE [--xtab-rows FIELD[:WIDTH[:BINS]]] [--xtab-cols FIELD[:WIDTH[:BINS]]] [--xtab-who served|unserved|arrived|all]: the outcome cross-tabulation
 * (prach_run_trials_xtab: reduced on the device, so it works with --logs 0), one group per sweep point with the --times seeds merged, labelled nUE; FIELD is
 * one of one, arrival, sojourn, completion, timer, ptc, failcount, age, state; the defaults — rows arrival:500 with as many bins as cover maxTime, columns
 * state:1:7, everybody — say what became of the UEs by when they arrived; --program beta|withnoma only, and not together with --cdf, --timeline, --sojourn,
 * --ci or --trace (one reduction per call);
 * --pick FILE [--pick-where FIELD:LO:HI]... [--pick-top FIELD | --pick-bottom FIELD] [--pick-k K] [--pick-who served|unserved|arrived|idle|all]: WHICH UEs stand
 * behind a count (prach_run_trials_pick: selected on the device, so it works with --logs 0): per trial of the grid, in trial order, a header line with the
 * exact number of matches and the K (default 16) UEs that pass every clause LO <= FIELD <= HI (at most 4) — the first K by index, or those with the largest
 * (--pick-top) / smallest (--pick-bottom) FIELD — as one line each: label nUE, trial, seed, nUE, rank, key, arrival and the 16 logged fields; --program
 * beta|withnoma only, and not together with --cdf, --timeline, --sojourn, --ci, --trace or --xtab (one reduction per call);
 * --census FILE [--census-rows FIELD[:WIDTH[:BINS]]] [--census-cols FIELD[:WIDTH[:BINS]]] [--census-who served|pending|dropped|arrived|all]: NOMA.c's outcome
 * census (prach_run_trials_noma_census: reduced on the device), one group per sweep point with the --times seeds merged, labelled nUE, in --xtab's line format;
 * FIELD is one of one, arrival, sojourn, completion, timer, ptc, retx, msg3fail, age, state, sector, preamble, lost (the NOMA menu of include/prach.h); the
 * defaults — rows arrival:500, columns state:1:9, everybody — say what became of the UEs by when they arrived; --program noma with Philox only, and not
 * together with another reduction;
 * --census-ci FILE [--census-ci-fields F1,F2,..] [--census-ci-who served|pending|dropped|arrived|all] [--census-ci-levels M1,..]: how far one seed lies from the
 * next, for NOMA.c (prach_run_trials_noma_summary: one row per trial, selected on the device; prach_noma_summary_stats in the parent, in trial order, so the
 * file does not depend on --gpus): per sweep point, labelled nUE, in --ci's line format, served_ratio, dropped_ratio, pending_ratio, restart_ratio and, per
 * field of the NOMA menu (at most 4; default sojourn,timer,ptc,lost) over the UEs of the class (default served), its mean and its exact order statistics at
 * the levels (permille, at most 8; default 500,950,990); --program noma with Philox only, and not together with another reduction;
 * --census-pick FILE [--census-pick-where FIELD:LO:HI]... [--census-pick-top FIELD | --census-pick-bottom FIELD] [--census-pick-k K] [--census-pick-who
 * served|pending|dropped|arrived|idle|all]: WHICH UEs stand behind a count of the census (prach_run_trials_noma_pick: selected on the device), --pick's lines
 * with fields of the NOMA menu: one header and at most K (default 16) rows per trial, in trial order; --program noma with Philox only, and not together with
 * another reduction;
 * --census-trace FILE [--census-trace-bin MS]: NOMA.c's channel trace (prach_run_trials_noma_trace: recorded by prach::noma_kernel while it runs and reduced on
 * the device) — per sector and all sectors, the preambles sent (tx), the (sector, preamble) bins used and alone (used, singles), the UEs granted, the
 * power-domain pairs and the pairs of which one UE decoded (pairs, pair_one), by time — one group per sweep point with the --times seeds merged, labelled nUE;
 * bins of MS ms (default 5) that cover maxTime; --program noma with Philox only, and not together with another reduction;
 * --census-timeline FILE [--census-timeline-bin MS]: NOMA.c's timeline per sector (prach_run_trials_noma_timeline: reduced on the device from the log records
 * prach::noma_kernel leaves there) — per sector and all sectors, the UEs that arrived, were served and were dropped, the sojourn and timer sums of the served,
 * all by ARRIVAL time, and the completions by completion time — on --census-trace's bins, so that the two files line up; one group per sweep point with the
 * --times seeds merged, labelled nUE; bins of MS ms (default 5) that cover maxTime + 6; --program noma with Philox only, and not together with another
 * reduction.  (A sojourn HISTOGRAM by arrival time is --census FILE --census-rows arrival:W:B --census-cols sojourn:W:B --census-who served);
 * --census-gain FILE [--census-gain-bins N] [--census-gain-width W] [--census-gain-lo L]: NOMA.c's near-far profile (prach_run_trials_noma_gain: reduced on the
 * device from the log records and the launch's own activation table) — per sector and all sectors, the UEs that arrived, were served and were dropped, and the
 * sojourn, lost-time and preamble-count sums of the served, by the UE's channel-gain LEVEL floor(1000 ln g): N bins (default 65, at most 4096) of W levels
 * (default 200) from level L on (default -16200: -162.00 ... -32.00 in 10 ln g, every gain a trial can draw); one group per sweep point with the --times seeds
 * merged, labelled nUE; --program noma with Philox only, and not together with another reduction;
 * --devices LIST: the same with explicit HIP ordinals (an ordinal may repeat);
 * --gpus N: the --times x sweep grid sharded over N devices of the node by host C — one forked child per device,
 * forked BEFORE any HIP call, trials dealt by descending cost (Philox: any trial anywhere; glibc: whole seeds, because
 * the sweep of a seed is chained through its rand() stream), results merged by the parent through shared memory; the
 * reference runs the grid serially (RandomAccessWithNOMA.c:216-221).
 */
#define _GNU_SOURCE
#include "prach_grouped.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

static void usage_and_exit(void) { /* text of WithNOMA:160-202 */
    printf("--times         -t : Simulation times (int)\n");
    printf("                     Simulation count must be greater than zero.\n");
    printf("                     Default 1\n\n");
    printf("--distribution  -d : Traffic model (1 or 2)\n");
    printf("                     1: traffic model 1 (Uniform distribution)\n");
    printf("                     2: traffic model 2 (Beta distribution)\n\n");
    printf("--preambles     -p : Number of preambles (int)\n");
    printf("                     Number of preamble must be greater than zero.\n");
    printf("                     Default 54\n\n");
    printf("--backoff       -b : Backoff indicator (int)\n");
    printf("                     Backoff indicator must be greater than zero.\n");
    printf("                     Default 20\n\n");
    printf("--grant         -g : The number of Up Link Grant per RAR (int)\n");
    printf("                     The number of Up Link Grant per RAR must be greater than zero.\n");
    printf("                     Default 12\n\n");
    printf("--rarCount      -r : RAR window size (int)\n");
    printf("                     The maximum RAR window size must be greater than zero.\n");
    printf("                     Default 5\n\n");
    printf("--maxRar        -m : Maximum retransmission (int)\n");
    printf("                     Maximum retransmissions must be greater than zero.\n");
    printf("                     Default 10\n\n");
    printf("--subframe      -s : Subframe units (int)\n");
    printf("                     The size of the subframe must be at least 5. (float)\n");
    printf("                     Default 5\n\n");
    printf("--cell          -c : Cell radius Size\n");
    printf("                     The radius of the cell is entered in diameter units and must be greater than 400m.\n");
    printf("                     Default 400.0\n\n");
    printf("--hbs           -b : Height of BS from ground (float)\n");
    printf("                     The height of the BS must be between 10m and 20m.\n");
    printf("                     Default 10.0\n\n");
    printf("--hut           -u : Height of UE from ground (float)\n");
    printf("                     The height of the UE must be between 1.5m and 22.5m.\n");
    printf("                     Default 1.8\n\n");
    exit(-1);
}

static int is(const char *a, const char *l, const char *s1, const char *s2) {
    return strcmp(a, l) == 0 || (s1 && strcmp(a, s1) == 0) || (s2 && strcmp(a, s2) == 0);
}
static void die(const char *msg) { printf("%s", msg); exit(-1); }


static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* The reduction a run makes on the device next to its results, never two of them.  A GROUPED kind (csrc/prach_grouped.h: --cdf, --timeline, --sojourn, --trace,
 * --xtab, --census, --census-trace, --census-timeline, --census-gain) is a block of groups, one group per sweep point; a block holds the groups of one worker or of one call:
 * the kind's structs [npts], then its arrays in the order of the C ABI, array q of all groups [npts][words of q] — e.g. --cdf prach_dist[npts] |
 * delay_hist[npts][bins] | ptc_hist[npts][256]; --sojourn prach_sojourn[npts] | hist[npts][rows][bins] | row_arrived[npts][rows] | row_delay_overflow[npts][rows].
 * The library's row of the kind says the sizes; shape, merge, run and CSV are the library's generic functions.  No kind, no per-trial spec: plain prach_run_trials. */
typedef struct reduction {
    int kind;         /* PRACH_G_*; -1: no block of groups */
    const void *spec; /* the kind's prach_*_spec */
    const char *path; /* the CSV file */
    size_t text_cap;  /* the CSV text of one group at most */
    /* --ci (prach_run_trials_summary) is no block of groups: one row per trial of the grid, in a shared mapping like the results; the parent computes the statistics */
    const prach_summary_spec *sm;
    prach_trial_summary *sm_rows;
    /* --pick (prach_run_trials_pick), like --ci: one header and k rows per trial of the grid, in shared mappings; the parent writes them in trial order */
    const prach_pick_spec *pk;
    prach_pick *pk_hdr;
    prach_pick_row *pk_rows;
    int pk_noma;                /* --census-pick: `pk` is over the NOMA menu (prach_run_trials_noma_pick) */
    /* --census-ci (prach_run_trials_noma_summary), like --ci: one row per trial of the grid in a shared mapping; the parent computes the statistics */
    const prach_noma_summary_spec *nsm;
    prach_noma_trial_summary *nsm_rows;
} reduction;
static int red_on(const reduction *r) { return r->kind >= 0; }
static size_t xt_cells(const prach_xtab_spec *s) { return ((size_t)s->row_bins + 1) * ((size_t)s->col_bins + 1); }
static size_t red_ngroups(const reduction *r) { return (size_t)*(const int32_t *)((const char *)r->spec + prach_internal_grouped_row(r->kind)->ngroups_at); }
static size_t red_block_bytes(const reduction *r) {
    size_t words[PRACH_G_MAX_ARRAYS], group = red_on(r) ? prach_internal_grouped_row(r->kind)->group_bytes : 0;
    const int na = red_on(r) ? prach_internal_grouped_shape(r->kind, r->spec, words) : 0;
    for (int q = 0; q < na; q++) group += 8 * words[q];
    return na ? red_ngroups(r) * group : 0;
}
/* group g of block b: its struct, and its q-th array */
static void *red_group(const reduction *r, char *b, int g) { return b + (size_t)g * prach_internal_grouped_row(r->kind)->group_bytes; }
static uint64_t *red_array(const reduction *r, char *b, int q, int g) {
    size_t words[PRACH_G_MAX_ARRAYS];
    prach_internal_grouped_shape(r->kind, r->spec, words);
    uint64_t *a = (uint64_t *)red_group(r, b, (int)red_ngroups(r));
    for (int i = 0; i < q; i++) a += red_ngroups(r) * words[i];
    return a + (size_t)g * words[q];
}
/* the arrays of group g of block b, as the library's generic functions take them; returns their number */
static int red_arrays(const reduction *r, char *b, int g, uint64_t *arrays[PRACH_G_MAX_ARRAYS]) {
    size_t words[PRACH_G_MAX_ARRAYS];
    const int na = prach_internal_grouped_shape(r->kind, r->spec, words);
    for (int q = 0; q < na; q++) arrays[q] = red_array(r, b, q, g);
    return na;
}
/* a zero-filled block becomes one of empty groups: a maximum over nothing is -1 */
static void red_init_block(const reduction *r, char *b) {
    const prach_grouped_row *k = prach_internal_grouped_row(r->kind);
    for (size_t g = 0; g < red_ngroups(r); g++)
        for (int m = 0; m < k->maxima; m++) ((int64_t *)red_group(r, b, (int)g))[k->counters + m] = -1;
}
static void red_merge_block(const reduction *r, char *into, char *from) {
    for (size_t g = 0; g < red_ngroups(r); g++) {
        uint64_t *a[PRACH_G_MAX_ARRAYS], *b[PRACH_G_MAX_ARRAYS];
        red_arrays(r, into, (int)g, a);
        red_arrays(r, from, (int)g, b);
        prach_internal_grouped_merge(r->kind, r->spec, red_group(r, into, (int)g), a, red_group(r, from, (int)g), (const uint64_t *const *)b);
    }
}
/* the CSV text of group g of block b; returns its length (>= cap: it did not fit) */
static size_t red_format_group(const reduction *r, char *b, int g, const char *label, char *out, size_t cap) {
    uint64_t *a[PRACH_G_MAX_ARRAYS];
    red_arrays(r, b, g, a);
    return prach_internal_grouped_format_csv(r->kind, r->spec, red_group(r, b, g), (const uint64_t *const *)a, label, out, cap);
}

/* FIELD[:WIDTH[:BINS]] of --xtab-rows / --xtab-cols.  Defaults: width 500 for arrival, otherwise 1; as many bins as cover max_time (arrival) or max_time + 6 (the
 * other times), 7 for state, 1 for one, 255 for ptc and failcount.  Returns 0 for a text that is none */
static const char *const xtab_names[PRACH_XTAB_NFIELDS] = {"one", "arrival", "sojourn", "completion", "timer", "ptc", "failcount", "age", "state"};
/* the field of the menu that the first `len` characters of `text` name; -1: none */
static int xtab_field(const char *text, size_t len) {
    for (int q = 0; q < PRACH_XTAB_NFIELDS; q++)
        if (strlen(xtab_names[q]) == len && strncasecmp(xtab_names[q], text, len) == 0) return q;
    return -1;
}
/* FIELD:LO:HI of --pick-where.  Returns 0 for a text that is none */
static int pick_clause(const char *text, prach_pick_clause *c) {
    const char *c1 = strchr(text, ':'), *c2 = c1 ? strchr(c1 + 1, ':') : NULL;
    if (!c2 || strchr(c2 + 1, ':')) return 0;
    const int f = xtab_field(text, (size_t)(c1 - text));
    char *end1, *end2;
    const long lo = strtol(c1 + 1, &end1, 10), hi = strtol(c2 + 1, &end2, 10);
    if (f < 0 || end1 != c2 || end1 == c1 + 1 || *end2 || end2 == c2 + 1 || lo < 0 || hi < lo || hi > INT32_MAX) return 0;
    c->field = f; c->lo = (int32_t)lo; c->hi = (int32_t)hi;
    return 1;
}
static int xtab_axis(const char *text, int max_time, int32_t *field, int32_t *width, int32_t *bins) {
    const char *c1 = strchr(text, ':'), *c2 = c1 ? strchr(c1 + 1, ':') : NULL;
    const size_t len = c1 ? (size_t)(c1 - text) : strlen(text);
    const int f = xtab_field(text, len);
    if (f < 0 || (c2 && strchr(c2 + 1, ':'))) return 0;
    const long w = c1 ? atol(c1 + 1) : f == PRACH_XTAB_ARRIVAL ? 500 : 1;
    if (w < 1 || w > INT32_MAX) return 0;
    long b = f == PRACH_XTAB_ONE ? 1 : f == PRACH_XTAB_STATE ? 7 : f == PRACH_XTAB_PTC || f == PRACH_XTAB_FAILCOUNT ? 255
             : (max_time + (f == PRACH_XTAB_ARRIVAL ? 0 : 6) + w - 1) / w;
    if (b > PRACH_XTAB_MAX_BINS) b = PRACH_XTAB_MAX_BINS;
    if (c2) b = atol(c2 + 1);
    if (b < 1 || b > PRACH_XTAB_MAX_BINS) return 0;
    *field = f; *width = (int32_t)w; *bins = (int32_t)b;
    return 1;
}

/* FIELD[:WIDTH[:BINS]] of --census-rows / --census-cols: a field of the NOMA menu.  Defaults: width 500 for arrival, otherwise 1; as many bins as cover max_time
 * (arrival) or max_time + 6 (the other times), 9 for state, 1 for one, 6 for sector, 64 for preamble, 255 for ptc, retx and msg3fail.  Returns 0 for a text that is none */
static const char *const noma_names[PRACH_NOMA_NFIELDS] = {"one", "arrival", "sojourn", "completion", "timer", "ptc", "retx", "msg3fail", "age", "state", "sector", "preamble", "lost"};
static int noma_field(const char *text, size_t len) {
    for (int q = 0; q < PRACH_NOMA_NFIELDS; q++)
        if (strlen(noma_names[q]) == len && strncasecmp(noma_names[q], text, len) == 0) return q;
    return -1;
}
/* FIELD:LO:HI of --census-pick-where.  Returns 0 for a text that is none */
static int noma_pick_clause(const char *text, prach_pick_clause *c) {
    const char *c1 = strchr(text, ':'), *c2 = c1 ? strchr(c1 + 1, ':') : NULL;
    if (!c2 || strchr(c2 + 1, ':')) return 0;
    const int f = noma_field(text, (size_t)(c1 - text));
    char *end1, *end2;
    const long lo = strtol(c1 + 1, &end1, 10), hi = strtol(c2 + 1, &end2, 10);
    if (f < 0 || end1 != c2 || end1 == c1 + 1 || *end2 || end2 == c2 + 1 || lo < 0 || hi < lo || hi > INT32_MAX) return 0;
    c->field = f; c->lo = (int32_t)lo; c->hi = (int32_t)hi;
    return 1;
}
/* the classes of --census-who, --census-ci-who and --census-pick-who (idle: the pick only); 0 for a text that is none */
static int noma_who(const char *t, int idle_too) {
    return strcmp(t, "served") == 0 ? PRACH_NOMA_SERVED : strcmp(t, "pending") == 0 ? PRACH_NOMA_PENDING : strcmp(t, "dropped") == 0 ? PRACH_NOMA_DROPPED
           : strcmp(t, "arrived") == 0 ? (PRACH_NOMA_SERVED | PRACH_NOMA_PENDING | PRACH_NOMA_DROPPED)
           : strcmp(t, "all") == 0 ? (PRACH_NOMA_SERVED | PRACH_NOMA_PENDING | PRACH_NOMA_DROPPED | PRACH_NOMA_IDLE)
           : idle_too && strcmp(t, "idle") == 0 ? PRACH_NOMA_IDLE : 0;
}
static int noma_axis(const char *text, int max_time, int32_t *field, int32_t *width, int32_t *bins) {
    const char *c1 = strchr(text, ':'), *c2 = c1 ? strchr(c1 + 1, ':') : NULL;
    const size_t len = c1 ? (size_t)(c1 - text) : strlen(text);
    const int f = noma_field(text, len);
    if (f < 0 || (c2 && strchr(c2 + 1, ':'))) return 0;
    const long w = c1 ? atol(c1 + 1) : f == PRACH_NOMA_ARRIVAL ? 500 : 1;
    if (w < 1 || w > INT32_MAX) return 0;
    long b = f == PRACH_NOMA_ONE ? 1 : f == PRACH_NOMA_STATE ? 9 : f == PRACH_NOMA_SECTOR ? 6 : f == PRACH_NOMA_PREAMBLE ? 64
             : f == PRACH_NOMA_PTC || f == PRACH_NOMA_RETX || f == PRACH_NOMA_MSG3FAIL ? 255 : (max_time + (f == PRACH_NOMA_ARRIVAL ? 0 : 6) + w - 1) / w;
    if (b > PRACH_XTAB_MAX_BINS) b = PRACH_XTAB_MAX_BINS;
    if (c2) b = atol(c2 + 1);
    if (b < 1 || b > PRACH_XTAB_MAX_BINS) return 0;
    *field = f; *width = (int32_t)w; *bins = (int32_t)b;
    return 1;
}

/* one call into the library with the run's reduction: its groups (group = sweep point, grp[k]) come back in call_block and are merged into the worker's block */
static int run_call(prach_engine *eng, const prach_cfg *c, int n, prach_result *r, prach_ue_log *const *logs, const reduction *red, const int32_t *grp,
                    char *call_block, char *worker_block, prach_trial_summary *sm_rows, prach_pick *pk_hdr, prach_pick_row *pk_rows, prach_noma_trial_summary *nsm_rows) {
    if (red->sm) return prach_run_trials_summary(eng, c, n, r, logs, red->sm, sm_rows);
    if (red->nsm) return prach_run_trials_noma_summary(eng, c, n, r, logs, red->nsm, nsm_rows);
    if (red->pk && red->pk_noma) return prach_run_trials_noma_pick(eng, c, n, r, logs, red->pk, pk_hdr, pk_rows);
    if (red->pk) return prach_run_trials_pick(eng, c, n, r, logs, red->pk, pk_hdr, pk_rows);
    if (!red_on(red)) return prach_run_trials(eng, c, n, r, logs);
    uint64_t *arrays[PRACH_G_MAX_ARRAYS];
    red_arrays(red, call_block, 0, arrays);
    const int rc = prach_internal_grouped_run(red->kind, eng, c, n, r, logs, red->spec, grp, call_block, arrays);
    if (rc == PRACH_OK) red_merge_block(red, worker_block, call_block);
    return rc;
}

/* One worker = one device: runs the trials idx[0..m) of the grid on `device` and leaves every prach_result in the (shared)
 * array `res`; per-trial files are written by the worker itself (independent files).  Philox trials go out in calls of up to
 * 1024 trials (one workgroup or cluster per trial); in glibc mode `idx` holds whole seeds in grid order and the sweep of a
 * seed is chained through cfg.stream_offset like the reference's single srand() per seed (WithNOMA:219-221): one call per
 * sweep point with all the worker's seeds in it.  Returns 0 or an exit code. */
static int run_worker(int device, const prach_cfg *cfgs, const int *idx, int m, prach_result *res, double *lat_out, int want_logs,
                      const char *outdir, int glibc, int npts, const reduction *red, char *worker_block) {
    const int reduces = red_on(red);
    prach_engine *eng = NULL;
    int rc = prach_engine_create(device, &eng);
    if (rc != PRACH_OK) { fprintf(stderr, "prach_sim: device %d: %s\n", device, prach_strerror(rc)); return 2; }
    const double t0 = now_s();
    const int CH = glibc ? m : 1024;
    prach_cfg *c = (prach_cfg *)malloc(sizeof(prach_cfg) * (size_t)(m > 0 ? m : 1));
    prach_result *r = (prach_result *)malloc(sizeof(prach_result) * (size_t)(m > 0 ? m : 1));
    prach_ue_log **logs = want_logs ? (prach_ue_log **)calloc((size_t)(m > 0 ? m : 1), sizeof(prach_ue_log *)) : NULL;
    if (!c || !r || (want_logs && !logs)) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    int32_t *grp = reduces ? (int32_t *)malloc(sizeof(int32_t) * (size_t)(m > 0 ? m : 1)) : NULL;
    char *call_block = reduces ? (char *)malloc(red_block_bytes(red)) : NULL;
    if (reduces && (!grp || !call_block)) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    prach_trial_summary *sr = red->sm ? (prach_trial_summary *)malloc(sizeof(prach_trial_summary) * (size_t)(m > 0 ? m : 1)) : NULL;
    if (red->sm && !sr) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    prach_noma_trial_summary *nsr = red->nsm ? (prach_noma_trial_summary *)malloc(sizeof(prach_noma_trial_summary) * (size_t)(m > 0 ? m : 1)) : NULL;
    if (red->nsm && !nsr) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    /* --pick: the headers and rows of one call (at most CH trials, or the worker's seeds) */
    const size_t pk_n = (size_t)(m < CH ? (m > 0 ? m : 1) : CH), pk_k = red->pk ? (size_t)red->pk->k : 0;
    prach_pick *ph = red->pk ? (prach_pick *)malloc(sizeof(prach_pick) * pk_n) : NULL;
    prach_pick_row *pr = red->pk ? (prach_pick_row *)malloc(sizeof(prach_pick_row) * pk_n * pk_k) : NULL;
    if (red->pk && (!ph || !pr)) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    if (!glibc) {
        for (int a = 0; a < m; a += CH) {
            const int n = m - a < CH ? m - a : CH;
            for (int k = 0; k < n; k++) {
                c[k] = cfgs[idx[a + k]];
                if (reduces) grp[k] = idx[a + k] % npts;
                if (want_logs) {
                    logs[k] = (prach_ue_log *)malloc(sizeof(prach_ue_log) * (size_t)c[k].nUE);
                    if (!logs[k]) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
                }
            }
            rc = run_call(eng, c, n, r, logs, red, grp, call_block, worker_block, sr, ph, pr, nsr);
            if (rc != PRACH_OK) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(rc)); return 2; }
            const double lat = now_s() - t0;
            for (int k = 0; k < n; k++) {
                res[idx[a + k]] = r[k];
                if (red->sm) red->sm_rows[idx[a + k]] = sr[k];
                if (red->nsm) red->nsm_rows[idx[a + k]] = nsr[k];
                if (red->pk) { red->pk_hdr[idx[a + k]] = ph[k]; memcpy(red->pk_rows + (size_t)idx[a + k] * pk_k, pr + (size_t)k * pk_k, sizeof(prach_pick_row) * pk_k); }
                lat_out[idx[a + k]] = lat;
                if (cfgs[idx[a + k]].variant != PRACH_VARIANT_NOMA_C) {
                    rc = prach_write_trial_files(&c[k], &r[k], want_logs ? logs[k] : NULL, lat, outdir);
                    if (rc != PRACH_OK) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(rc)); return 2; }
                }
                if (want_logs) { free(logs[k]); logs[k] = NULL; }
            }
        }
    } else { /* idx = seeds' trials in grid order: idx[s * npts + k]; chained per seed */
        const int nseeds = m / npts;
        uint64_t *offset = (uint64_t *)calloc((size_t)(nseeds > 0 ? nseeds : 1), sizeof(uint64_t));
        if (!offset) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int k = 0; k < npts; k++) {
            for (int s_ = 0; s_ < nseeds; s_++) {
                c[s_] = cfgs[idx[s_ * npts + k]];
                c[s_].stream_offset = offset[s_];
                if (reduces) grp[s_] = k;
                if (want_logs) {
                    logs[s_] = (prach_ue_log *)malloc(sizeof(prach_ue_log) * (size_t)c[s_].nUE);
                    if (!logs[s_]) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
                }
            }
            rc = run_call(eng, c, nseeds, r, logs, red, grp, call_block, worker_block, sr, ph, pr, nsr);
            if (rc != PRACH_OK) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(rc)); return 2; }
            const double lat = now_s() - t0;
            for (int s_ = 0; s_ < nseeds; s_++) {
                offset[s_] += r[s_].draws;
                res[idx[s_ * npts + k]] = r[s_];
                if (red->sm) red->sm_rows[idx[s_ * npts + k]] = sr[s_];
                if (red->nsm) red->nsm_rows[idx[s_ * npts + k]] = nsr[s_];
                if (red->pk) { red->pk_hdr[idx[s_ * npts + k]] = ph[s_]; memcpy(red->pk_rows + (size_t)idx[s_ * npts + k] * pk_k, pr + (size_t)s_ * pk_k, sizeof(prach_pick_row) * pk_k); }
                lat_out[idx[s_ * npts + k]] = lat;
                if (c[s_].variant != PRACH_VARIANT_NOMA_C) { /* (NOMA.c's lines are printed and appended by the parent) */
                    rc = prach_write_trial_files(&c[s_], &r[s_], want_logs ? logs[s_] : NULL, lat, outdir);
                    if (rc != PRACH_OK) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(rc)); return 2; }
                }
                if (want_logs) { free(logs[s_]); logs[s_] = NULL; }
            }
        }
        free(offset);
    }
    free(c); free(r); free(logs); free(grp); free(call_block); free(sr); free(nsr); free(ph); free(pr);
    prach_engine_destroy(eng);
    return 0;
}

int main(int argc, char *argv[]) {
    int randomMax = 1, variant = PRACH_VARIANT_WITHNOMA_C, rng = PRACH_RNG_GLIBC, device = 0, want_logs = 1, gpus = 1, rng_given = 0;
    int sweep_lo = 10000, sweep_hi = 100000, sweep_step = 10000; /* WithNOMA:221 */
    const char *outdir = ".", *csv_path = NULL, *devlist = NULL, *cdf_path = NULL, *tl_path = NULL, *sj_path = NULL, *ci_path = NULL, *tr_path = NULL, *xt_path = NULL, *pk_path = NULL;
    const char *pk_who = "all";
    prach_pick_spec pk_spec = {0, 0, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, PRACH_PICK_BY_INDEX, PRACH_XTAB_ONE, 16, 0};
    const char *xt_rows = "arrival:500", *xt_cols = "state:1:7", *xt_who = "all";
    const char *nc_path = NULL, *nc_rows = "arrival:500", *nc_cols = "state:1:9", *nc_who = "all";
    prach_summary_spec ci_spec = {3, {500, 950, 990, 0, 0, 0, 0, 0}, {0, 0, 0}};
    /* --census-ci, --census-pick (--program noma) */
    const char *nci_path = NULL, *nci_who = "served", *npk_path = NULL, *npk_who = "all";
    prach_noma_summary_spec nci_spec = {0, 4, {PRACH_NOMA_SOJOURN, PRACH_NOMA_TIMER, PRACH_NOMA_PTC, PRACH_NOMA_LOST}, 3, {500, 950, 990, 0, 0, 0, 0, 0}, {0, 0}};
    prach_pick_spec npk_spec = {0, 0, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, PRACH_PICK_BY_INDEX, PRACH_NOMA_ONE, 16, 0};
    int cdf_bins = 4096, cdf_bin_ms = 1, tl_bin_ms = 5, sj_row_ms = 500, sj_bin_ms = 5, tr_bin_ms = 5, ntr_bin_ms = 5, ntl_bin_ms = 5;
    const char *ntr_path = NULL, *ntl_path = NULL, *ng_path = NULL;
    int ng_bins = 65, ng_width = 200, ng_lo = -16200;
    int devs[64];
    /* --program must be known before the defaults are laid down */
    for (int i = 1; i + 1 < argc; i += 2)
        if (strcmp(argv[i], "--program") == 0)
            variant = strcmp(argv[i + 1], "beta") == 0 ? PRACH_VARIANT_BETA_C : (strcmp(argv[i + 1], "noma") == 0 ? PRACH_VARIANT_NOMA_C : PRACH_VARIANT_WITHNOMA_C);
    prach_cfg base;
    prach_cfg_defaults(&base, variant);
    if (variant == PRACH_VARIANT_NOMA_C) { randomMax = 10; rng = PRACH_RNG_PHILOX; want_logs = 0; } /* NOMA.c:644 */

    for (int i = 1; i < argc; i += 2) {
        const char *a = argv[i];
        if (i + 1 >= argc) usage_and_exit(); /* the reference dereferences NULL here; we print the usage */
        const char *v = argv[i + 1];
        if (is(a, "--times", "-t", NULL)) {
            if (atoi(v) < 1) die("Simulation count must be greater than zero.");
            randomMax = atoi(v);
        } else if (is(a, "--distribution", "-d", NULL)) {
            if (atoi(v) != 1 && atoi(v) != 0 && atoi(v) != 2) die("Traffic model just choose 1 or 2");
            base.uniform = atoi(v) == 1;
        } else if (is(a, "--preambles", "-p", NULL)) {
            if (atoi(v) < 1) die("Number of preamble must be greater than zero.");
            base.nPreamble = atoi(v);
        } else if (is(a, "--backoff", "-b", NULL)) {
            if (atoi(v) < 1) die("Backoff indicator must be greater than zero.");
            base.backoff = atoi(v);
        } else if (is(a, "--grant", "-g", NULL)) {
            if (atoi(v) < 1) die("The number of Up Link Grant per RAR must be greater than zero.");
            base.nGrantUL = atoi(v);
        } else if (is(a, "--rarCount", "-rc", "-r")) {
            if (atoi(v) < 1) die("The maximum RAR window size must be greater than zero.");
            base.maxRarWindow = atoi(v) + 1; /* WithNOMA:128 */
        } else if (is(a, "--maxRar", "-mrc", "-m")) {
            if (atoi(v) < 1) die("Maximum retransmissions must be greater than zero.");
            base.maxMsg2TxCount = atoi(v) - 1; /* WithNOMA:134 */
        } else if (is(a, "--subframe", "-s", NULL)) {
            if (atoi(v) < 5) die("The size of the subframe must be at least 5.");
            base.accessTime = atoi(v);
        } else if (is(a, "--cell", "-c", NULL)) {
            if (atof(v) < 400.0) die("The radius of the cell is entered in diameter units and must be greater than 400m.");
            base.cellRadius = (float)atof(v);
        } else if (is(a, "--hbs", "-bs", NULL)) {
            if (atof(v) < 10.0 || atof(v) > 20.0) die("The height of the BS must be between 10m and 20m.");
            base.hBS = (float)atof(v);
        } else if (is(a, "--hut", "-ut", "-u")) {
            if (atof(v) < 1.5 || atof(v) > 22.5) die("The height of the UE must be between 1.5m and 22.5m.");
            base.hUT = (float)atof(v);
        } else if (strcmp(a, "--program") == 0) {
            /* handled above */
        } else if (strcmp(a, "--rng") == 0) {
            rng = strcmp(v, "philox") == 0 ? PRACH_RNG_PHILOX : PRACH_RNG_GLIBC;
            rng_given = 1;
        } else if (strcmp(a, "--nue") == 0) {
            if (atoi(v) < 1) die("Number of UEs must be greater than zero.");
            sweep_lo = sweep_hi = atoi(v); sweep_step = 1;
        } else if (strcmp(a, "--sweep") == 0) {
            if (sscanf(v, "%d:%d:%d", &sweep_lo, &sweep_hi, &sweep_step) != 3 || sweep_lo < 1 || sweep_step < 1 || sweep_hi < sweep_lo)
                die("--sweep LO:HI:STEP");
        } else if (strcmp(a, "--out") == 0) {
            outdir = v;
        } else if (strcmp(a, "--logs") == 0) {
            want_logs = atoi(v) != 0;
        } else if (strcmp(a, "--device") == 0) {
            device = atoi(v);
        } else if (strcmp(a, "--sector-grants") == 0) { /* the author's commented-out per-sector grant path (WithNOMA:312,626-637) */
            if (atoi(v)) base.flags |= PRACH_FLAG_SECTOR_GRANTS;
        } else if (strcmp(a, "--nonsector") == 0) { /* the author's commented-out cell-wide NOMA grouping (NOMA.c:688) */
            if (atoi(v)) base.flags |= PRACH_FLAG_NOMA_NONSECTOR;
        } else if (strcmp(a, "--gpus") == 0) {
            if (atoi(v) < 1 || atoi(v) > 64) die("--gpus N: 1..64 devices of this node");
            gpus = atoi(v);
        } else if (strcmp(a, "--devices") == 0) { /* explicit HIP ordinals, e.g. 0,2,3 (an ordinal may repeat: workers then share that device) */
            devlist = v;
        } else if (strcmp(a, "--csv") == 0) {
            csv_path = v;
        } else if (strcmp(a, "--cdf") == 0) {
            cdf_path = v;
        } else if (strcmp(a, "--cdf-bins") == 0) {
            if (atoi(v) < 1 || atoi(v) > PRACH_DIST_MAX_DELAY_BINS) die("--cdf-bins N: 1..16384 delay bins");
            cdf_bins = atoi(v);
        } else if (strcmp(a, "--cdf-bin-ms") == 0) {
            if (atoi(v) < 1) die("--cdf-bin-ms W: the width of a delay bin in ms, at least 1");
            cdf_bin_ms = atoi(v);
        } else if (strcmp(a, "--timeline") == 0) {
            tl_path = v;
        } else if (strcmp(a, "--timeline-bin") == 0) {
            if (atoi(v) < 1) die("--timeline-bin MS: the width of a timeline bin in ms, at least 1");
            tl_bin_ms = atoi(v);
        } else if (strcmp(a, "--sojourn") == 0) {
            sj_path = v;
        } else if (strcmp(a, "--sojourn-arrival-ms") == 0) {
            if (atoi(v) < 1) die("--sojourn-arrival-ms MS: the width of an arrival row in ms, at least 1");
            sj_row_ms = atoi(v);
        } else if (strcmp(a, "--sojourn-bin") == 0) {
            if (atoi(v) < 1) die("--sojourn-bin MS: the width of a delay bin in ms, at least 1");
            sj_bin_ms = atoi(v);
        } else if (strcmp(a, "--trace") == 0) {
            tr_path = v;
        } else if (strcmp(a, "--trace-bin") == 0) {
            if (atoi(v) < 1) die("--trace-bin MS: the width of a trace bin in ms, at least 1");
            tr_bin_ms = atoi(v);
        } else if (strcmp(a, "--xtab") == 0) {
            xt_path = v;
        } else if (strcmp(a, "--xtab-rows") == 0) {
            xt_rows = v;
        } else if (strcmp(a, "--xtab-cols") == 0) {
            xt_cols = v;
        } else if (strcmp(a, "--xtab-who") == 0) {
            xt_who = v;
        } else if (strcmp(a, "--census-gain") == 0) {
            ng_path = v;
        } else if (strcmp(a, "--census-gain-bins") == 0) {
            if (atoi(v) < 1 || atoi(v) > PRACH_NOMA_GAIN_MAX_BINS) die("--census-gain-bins N: the number of gain-level bins, 1 to 4096");
            ng_bins = atoi(v);
        } else if (strcmp(a, "--census-gain-width") == 0) {
            if (atoi(v) < 1) die("--census-gain-width W: the width of a gain-level bin in levels (hundredths of 10 ln g), at least 1");
            ng_width = atoi(v);
        } else if (strcmp(a, "--census-gain-lo") == 0) {
            ng_lo = atoi(v);
        } else if (strcmp(a, "--census-timeline") == 0) {
            ntl_path = v;
        } else if (strcmp(a, "--census-timeline-bin") == 0) {
            if (atoi(v) < 1) die("--census-timeline-bin MS: the width of a timeline bin in ms, at least 1");
            ntl_bin_ms = atoi(v);
        } else if (strcmp(a, "--census-trace") == 0) {
            ntr_path = v;
        } else if (strcmp(a, "--census-trace-bin") == 0) {
            if (atoi(v) < 1) die("--census-trace-bin MS: the width of a trace bin in ms, at least 1");
            ntr_bin_ms = atoi(v);
        } else if (strcmp(a, "--census") == 0) {
            nc_path = v;
        } else if (strcmp(a, "--census-rows") == 0) {
            nc_rows = v;
        } else if (strcmp(a, "--census-cols") == 0) {
            nc_cols = v;
        } else if (strcmp(a, "--census-who") == 0) {
            nc_who = v;
        } else if (strcmp(a, "--census-ci") == 0) {
            nci_path = v;
        } else if (strcmp(a, "--census-ci-who") == 0) {
            nci_who = v;
        } else if (strcmp(a, "--census-ci-fields") == 0) {
            nci_spec.nfields = 0;
            memset(nci_spec.field, 0, sizeof nci_spec.field);
            for (const char *q = v; *q;) {
                const char *e = strchr(q, ',') ? strchr(q, ',') : q + strlen(q);
                const int f = noma_field(q, (size_t)(e - q));
                if (nci_spec.nfields >= PRACH_NOMA_SUMMARY_MAX_FIELDS || f < 0) die("--census-ci-fields LIST: 1 to 4 comma-separated fields of the NOMA menu");
                nci_spec.field[nci_spec.nfields++] = f;
                q = *e ? e + 1 : e;
            }
            if (nci_spec.nfields < 1) die("--census-ci-fields LIST: 1 to 4 comma-separated fields of the NOMA menu");
        } else if (strcmp(a, "--census-ci-levels") == 0) {
            nci_spec.nq = 0;
            memset(nci_spec.permille, 0, sizeof nci_spec.permille);
            for (const char *q = v; *q;) {
                const int m_ = atoi(q);
                if (nci_spec.nq >= PRACH_SUMMARY_MAX_Q || m_ < 1 || m_ > 1000) die("--census-ci-levels LIST: 1 to 8 comma-separated levels in permille, 1 to 1000 each");
                nci_spec.permille[nci_spec.nq++] = m_;
                while (*q && *q != ',') q++;
                if (*q == ',') q++;
            }
            if (nci_spec.nq < 1) die("--census-ci-levels LIST: 1 to 8 comma-separated levels in permille, 1 to 1000 each");
        } else if (strcmp(a, "--census-pick") == 0) {
            npk_path = v;
        } else if (strcmp(a, "--census-pick-where") == 0) {
            if (npk_spec.nclauses >= PRACH_PICK_MAX_CLAUSES || !noma_pick_clause(v, &npk_spec.clause[npk_spec.nclauses])) die("--census-pick-where FIELD:LO:HI: a field of the NOMA menu, 0 <= LO <= HI, at most 4 clauses");
            npk_spec.nclauses++;
        } else if (strcmp(a, "--census-pick-top") == 0 || strcmp(a, "--census-pick-bottom") == 0) {
            if (npk_spec.order != PRACH_PICK_BY_INDEX || noma_field(v, strlen(v)) < 0) die("--census-pick-top FIELD or --census-pick-bottom FIELD: one of them, with a field of the NOMA menu");
            npk_spec.order = strcmp(a, "--census-pick-top") == 0 ? PRACH_PICK_LARGEST : PRACH_PICK_SMALLEST;
            npk_spec.key_field = noma_field(v, strlen(v));
        } else if (strcmp(a, "--census-pick-k") == 0) {
            if (atoi(v) < 1 || atoi(v) > PRACH_PICK_MAX_K) die("--census-pick-k K: 1..4096 UEs per trial");
            npk_spec.k = atoi(v);
        } else if (strcmp(a, "--census-pick-who") == 0) {
            npk_who = v;
        } else if (strcmp(a, "--pick") == 0) {
            pk_path = v;
        } else if (strcmp(a, "--pick-where") == 0) {
            if (pk_spec.nclauses >= PRACH_PICK_MAX_CLAUSES || !pick_clause(v, &pk_spec.clause[pk_spec.nclauses])) die("--pick-where FIELD:LO:HI: a field of the menu, 0 <= LO <= HI, at most 4 clauses");
            pk_spec.nclauses++;
        } else if (strcmp(a, "--pick-top") == 0 || strcmp(a, "--pick-bottom") == 0) {
            if (pk_spec.order != PRACH_PICK_BY_INDEX || xtab_field(v, strlen(v)) < 0) die("--pick-top FIELD or --pick-bottom FIELD: one of them, with a field of the menu");
            pk_spec.order = strcmp(a, "--pick-top") == 0 ? PRACH_PICK_LARGEST : PRACH_PICK_SMALLEST;
            pk_spec.key_field = xtab_field(v, strlen(v));
        } else if (strcmp(a, "--pick-k") == 0) {
            if (atoi(v) < 1 || atoi(v) > PRACH_PICK_MAX_K) die("--pick-k K: 1..4096 UEs per trial");
            pk_spec.k = atoi(v);
        } else if (strcmp(a, "--pick-who") == 0) {
            pk_who = v;
        } else if (strcmp(a, "--ci") == 0) {
            ci_path = v;
        } else if (strcmp(a, "--ci-levels") == 0) {
            ci_spec.nq = 0;
            for (const char *q = v; *q;) {
                const int m_ = atoi(q);
                if (ci_spec.nq >= PRACH_SUMMARY_MAX_Q || m_ < 1 || m_ > 1000) die("--ci-levels LIST: 1 to 8 comma-separated levels in permille, 1 to 1000 each");
                ci_spec.permille[ci_spec.nq++] = m_;
                while (*q && *q != ',') q++;
                if (*q == ',') q++;
            }
            if (ci_spec.nq < 1) die("--ci-levels LIST: 1 to 8 comma-separated levels in permille, 1 to 1000 each");
        } else {
            usage_and_exit();
        }
    }
    base.rng_mode = rng;
    if (ng_path && variant != PRACH_VARIANT_NOMA_C) die("--census-gain needs --program noma (the other programs draw no channel gain)");
    if (ng_path && (ntl_path || ntr_path || nci_path || npk_path || nc_path || pk_path || xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--census-gain cannot be combined with another reduction: one reduction per call");
    if (ng_path && rng_given && rng == PRACH_RNG_GLIBC) die("--census-gain needs --rng philox (NOMA.c in the reference's stream is not wired to the NOMA menu's device calls)");
    if (ntl_path && variant != PRACH_VARIANT_NOMA_C) die("--census-timeline needs --program noma (the other programs have --timeline)");
    if (ntl_path && (ntr_path || nci_path || npk_path || nc_path || pk_path || xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--census-timeline cannot be combined with another reduction: one reduction per call");
    if (ntl_path && rng_given && rng == PRACH_RNG_GLIBC) die("--census-timeline needs --rng philox (NOMA.c in the reference's stream is not wired to the NOMA menu's device calls)");
    if (ntr_path && variant != PRACH_VARIANT_NOMA_C) die("--census-trace needs --program noma (the other programs have --trace)");
    if (ntr_path && (nci_path || npk_path || nc_path || pk_path || xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--census-trace cannot be combined with another reduction: one reduction per call");
    if (ntr_path && rng_given && rng == PRACH_RNG_GLIBC) die("--census-trace needs --rng philox (NOMA.c in the reference's stream is not wired to the NOMA menu's device calls)");
    if (nci_path && variant != PRACH_VARIANT_NOMA_C) die("--census-ci needs --program noma (the other programs have --ci)");
    if (npk_path && variant != PRACH_VARIANT_NOMA_C) die("--census-pick needs --program noma (the other programs have --pick)");
    if (nci_path && (npk_path || nc_path || pk_path || xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--census-ci cannot be combined with --cdf, --timeline, --sojourn, --ci, --trace, --xtab, --pick, --census or --census-pick: one reduction per call");
    if (npk_path && (nc_path || pk_path || xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--census-pick cannot be combined with --cdf, --timeline, --sojourn, --ci, --trace, --xtab, --pick or --census: one reduction per call");
    if (nci_path && rng_given && rng == PRACH_RNG_GLIBC) die("--census-ci needs --rng philox (NOMA.c in the reference's stream is not wired to the NOMA menu's device calls)");
    if (npk_path && rng_given && rng == PRACH_RNG_GLIBC) die("--census-pick needs --rng philox (NOMA.c in the reference's stream is not wired to the NOMA menu's device calls)");
    if (nc_path && variant != PRACH_VARIANT_NOMA_C) die("--census needs --program noma (the other programs have --xtab)");
    if (nc_path && (pk_path || xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--census cannot be combined with --cdf, --timeline, --sojourn, --ci, --trace, --xtab or --pick: one reduction per call");
    if (nc_path && rng_given && rng == PRACH_RNG_GLIBC) die("--census needs --rng philox (NOMA.c in the reference's stream is not wired to the NOMA menu's device calls)");
    if (pk_path && (xt_path || tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--pick cannot be combined with --cdf, --timeline, --sojourn, --ci, --trace or --xtab: one reduction per call");
    if (pk_path && variant == PRACH_VARIANT_NOMA_C) die("--pick needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)");
    if (xt_path && (tr_path || ci_path || sj_path || tl_path || cdf_path)) die("--xtab cannot be combined with --cdf, --timeline, --sojourn, --ci or --trace: one reduction per call");
    if (xt_path && variant == PRACH_VARIANT_NOMA_C) die("--xtab needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)");
    if (tr_path && (ci_path || sj_path || tl_path || cdf_path)) die("--trace cannot be combined with --cdf, --timeline, --sojourn or --ci: one reduction per call");
    if (tr_path && variant == PRACH_VARIANT_NOMA_C) die("--trace needs --program beta or withnoma (NOMA.c's resolver is another one)");
    if (ci_path && variant == PRACH_VARIANT_NOMA_C) die("--ci needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)");
    if (ci_path && (sj_path || tl_path || cdf_path)) die("--ci cannot be combined with --cdf, --timeline or --sojourn: one reduction per call");
    if (sj_path && variant == PRACH_VARIANT_NOMA_C) die("--sojourn needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)");
    if (sj_path && (tl_path || cdf_path)) die("--sojourn cannot be combined with --cdf or --timeline: one reduction per call");
    if (tl_path && variant == PRACH_VARIANT_NOMA_C) die("--timeline needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)");
    if (tl_path && cdf_path) die("--timeline and --cdf cannot be combined: one reduction per call");
    if (csv_path && variant != PRACH_VARIANT_BETA_C) die("--csv needs --program beta (AveragePerformance.py reads its six-number Results.txt)");
    if (variant == PRACH_VARIANT_NOMA_C) { want_logs = 0; if (!rng_given) rng = PRACH_RNG_PHILOX; base.rng_mode = rng; } /* --rng glibc: NOMA.c's own rand() stream */

    /* the grid: trial (seed s, sweep point k) = cfgs[s * npts + k], the reference's loop order (WithNOMA:216-221 / NOMA.c:644-647) */
    const int npts = (sweep_hi - sweep_lo) / sweep_step + 1;
    const int ntr = randomMax * npts;
    const int glibc = rng == PRACH_RNG_GLIBC;
    prach_cfg *cfgs = (prach_cfg *)malloc(sizeof(prach_cfg) * (size_t)ntr);
    /* results and per-trial latencies live in shared memory: the workers (children) fill them, the parent prints and merges */
    prach_result *res = (prach_result *)mmap(NULL, sizeof(prach_result) * (size_t)ntr, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    double *lat = (double *)mmap(NULL, sizeof(double) * (size_t)ntr, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (!cfgs || res == MAP_FAILED || lat == MAP_FAILED) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    for (int s_ = 0; s_ < randomMax; s_++)
        for (int k = 0; k < npts; k++) {
            prach_cfg *c = &cfgs[s_ * npts + k];
            *c = base;
            c->nUE = sweep_lo + k * sweep_step;
            c->seed = (uint64_t)s_;
        }
    if (variant == PRACH_VARIANT_NOMA_C) {
        char path[1024];
        snprintf(path, sizeof path, "%s/TestResults", outdir);
        mkdir(path, 0755);
    } else {
        if (base.uniform) printf("Traffic model: Uniform\n\n"); /* WithNOMA:208-213 */
        else printf("Traffic model: Beta\n\n");
        fflush(stdout);
    }

    /* deal the trials to the workers: longest first onto the least loaded (cost = prach_trial_cost, a measured table); glibc mode deals whole seeds */
    if (devlist) {
        gpus = 0;
        for (const char *q = devlist; *q && gpus < 64;) {
            devs[gpus++] = atoi(q);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
        if (gpus < 1) die("--devices LIST: comma-separated HIP ordinals");
    } else {
        for (int w = 0; w < 64; w++) devs[w] = device + w;
    }
    if (gpus > ntr) gpus = ntr;
    if (glibc && gpus > randomMax) gpus = randomMax;
    int **widx = (int **)calloc((size_t)gpus, sizeof(int *));
    int *wn = (int *)calloc((size_t)gpus, sizeof(int));
    double *wload = (double *)calloc((size_t)gpus, sizeof(double));
    if (!widx || !wn || !wload) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    for (int w = 0; w < gpus; w++) {
        widx[w] = (int *)malloc(sizeof(int) * (size_t)ntr);
        if (!widx[w]) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
    }
    if (glibc) {
        for (int s_ = 0; s_ < randomMax; s_++) { /* seeds cost the same: round robin keeps every worker's seeds in grid order */
            const int w = s_ % gpus;
            for (int k = 0; k < npts; k++) widx[w][wn[w]++] = s_ * npts + k;
        }
    } else {
        for (int k = npts - 1; k >= 0; k--) /* sweep points are ascending in nUE: descending cost */
            for (int s_ = 0; s_ < randomMax; s_++) {
                int best = 0;
                for (int w = 1; w < gpus; w++) if (wload[w] < wload[best]) best = w;
                widx[best][wn[best]++] = s_ * npts + k;
                wload[best] += prach_trial_cost(&cfgs[s_ * npts + k]);
            }
    }

    /* --cdf / --timeline / --sojourn: one block of groups per worker in a shared mapping, like the results; the parent merges them (integers: exact in any order).
     * The timeline's bins cover the horizon (a completion is at most maxTime + 5) */
    const prach_dist_spec cdf_spec = {cdf_bins, cdf_bin_ms, npts, 0};
    const int tl_bins = (prach_max_time(&base) + 6 + tl_bin_ms - 1) / tl_bin_ms;
    const prach_timeline_spec tl_spec = {tl_bins, tl_bin_ms, npts, 0};
    if (tl_path && tl_bins > PRACH_TIMELINE_MAX_BINS) die("--timeline-bin MS: too many bins");
    /* the sojourn's rows cover the arrivals (below maxTime), its delay bins the horizon */
    const int sj_rows = (prach_max_time(&base) + sj_row_ms - 1) / sj_row_ms, sj_bins = (prach_max_time(&base) + 6 + sj_bin_ms - 1) / sj_bin_ms;
    const prach_sojourn_spec sj_spec = {sj_rows, sj_row_ms, sj_bins, sj_bin_ms, npts, 0};
    if (sj_path && sj_rows > PRACH_SOJOURN_MAX_ARRIVAL_BINS) die("--sojourn-arrival-ms MS: too many rows");
    if (sj_path && sj_bins > PRACH_SOJOURN_MAX_DELAY_BINS) die("--sojourn-bin MS: too many bins");
    /* a line of --cdf: a label of at most 10 digits, three numbers, a share; of --timeline: the label, a series name, two numbers; of --sojourn: the label and
     * three numbers, per cell and twice per row */
    const reduction red_ = {sj_path ? PRACH_G_SOJOURN : tl_path ? PRACH_G_TIMELINE : cdf_path ? PRACH_G_DIST : -1,
                            sj_path ? (const void *)&sj_spec : tl_path ? (const void *)&tl_spec : (const void *)&cdf_spec, sj_path ? sj_path : tl_path ? tl_path : cdf_path,
                            sj_path ? 64 * ((size_t)sj_rows * ((size_t)sj_bins + 2) + 1) + 1
                            : tl_path ? 64 * (5 * (size_t)tl_bins + 2) + 1 : 64 * ((size_t)cdf_bins + PRACH_DIST_PTC_BINS + 1) + 1, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL};
    reduction red_ci = red_;
    /* the trace's bins cover maxTime */
    const int tr_bins = (prach_max_time(&base) + tr_bin_ms - 1) / tr_bin_ms;
    const prach_trace_spec tr_spec = {tr_bins, tr_bin_ms, npts, 0};
    if (tr_path && tr_bins > PRACH_TRACE_MAX_BINS) die("--trace-bin MS: too many bins");
    if (tr_path) { red_ci.kind = PRACH_G_TRACE; red_ci.spec = &tr_spec; red_ci.path = tr_path; red_ci.text_cap = 64 * (4 * (size_t)tr_bins + 1) + 1; } /* (a line: the label, a series name, two numbers) */
    /* --census-trace: the same for NOMA.c's channel trace */
    const int ntr_bins = (prach_max_time(&base) + ntr_bin_ms - 1) / ntr_bin_ms;
    const prach_noma_trace_spec ntr_spec = {ntr_bins, ntr_bin_ms, npts, 0};
    if (ntr_path && ntr_bins > PRACH_TRACE_MAX_BINS) die("--census-trace-bin MS: too many bins");
    if (ntr_path && 36 * (uint64_t)npts * (uint64_t)ntr_bins > (1ull << 27)) die("--census-trace: too many bins for this many sweep points");
    /* --census-timeline: the same for NOMA.c's timeline per sector; its bins cover the completions too (maxTime + 6) */
    const int ntl_bins = (prach_max_time(&base) + 6 + ntl_bin_ms - 1) / ntl_bin_ms;
    const prach_noma_timeline_spec ntl_spec = {ntl_bins, ntl_bin_ms, npts, 0};
    if (ntl_path && ntl_bins > PRACH_TIMELINE_MAX_BINS) die("--census-timeline-bin MS: too many bins");
    if (ntl_path && 36 * (uint64_t)npts * (uint64_t)ntl_bins > (1ull << 27)) die("--census-timeline: too many bins for this many sweep points");
    if (ntl_path) { red_ci.kind = PRACH_G_NOMA_TIMELINE; red_ci.spec = &ntl_spec; red_ci.path = ntl_path; red_ci.text_cap = 80 * (6 * 7 * (size_t)ntl_bins + 2) + 1; } /* (a line: the label, a series name, a sector, two numbers) */
    /* --census-gain: NOMA.c's near-far profile per sector */
    const prach_noma_gain_spec ng_spec = {ng_bins, ng_width, ng_lo, npts, 0};
    if (ng_path && 36 * (uint64_t)npts * (uint64_t)ng_bins > (1ull << 27)) die("--census-gain: too many bins for this many sweep points");
    if (ng_path) { red_ci.kind = PRACH_G_NOMA_GAIN; red_ci.spec = &ng_spec; red_ci.path = ng_path; red_ci.text_cap = 80 * (6 * 7 * (size_t)ng_bins + 2) + 1; } /* (a line: the label, a series name, a sector, two numbers) */
    if (ntr_path) { red_ci.kind = PRACH_G_NOMA_TRACE; red_ci.spec = &ntr_spec; red_ci.path = ntr_path; red_ci.text_cap = 80 * (6 * 7 * (size_t)ntr_bins + 1) + 1; } /* (a line: the label, a series name, a sector, two numbers) */
    /* --xtab: the axes as given, the defaults of a field where width or bins are left out */
    prach_xtab_spec xt_spec = {0, 0, 0, 0, 0, 0, 0, npts, {0, 0}};
    if (xt_path) {
        xt_spec.who = strcmp(xt_who, "served") == 0 ? PRACH_XTAB_SERVED : strcmp(xt_who, "unserved") == 0 ? PRACH_XTAB_UNSERVED
                      : strcmp(xt_who, "arrived") == 0 ? (PRACH_XTAB_SERVED | PRACH_XTAB_UNSERVED) : strcmp(xt_who, "all") == 0 ? (PRACH_XTAB_SERVED | PRACH_XTAB_UNSERVED | PRACH_XTAB_IDLE) : 0;
        if (!xt_spec.who) die("--xtab-who served|unserved|arrived|all");
        if (!xtab_axis(xt_rows, prach_max_time(&base), &xt_spec.row_field, &xt_spec.row_width, &xt_spec.row_bins)) die("--xtab-rows FIELD[:WIDTH[:BINS]]: a field of the menu, a width of at least 1, 1 to 65536 bins");
        if (!xtab_axis(xt_cols, prach_max_time(&base), &xt_spec.col_field, &xt_spec.col_width, &xt_spec.col_bins)) die("--xtab-cols FIELD[:WIDTH[:BINS]]: a field of the menu, a width of at least 1, 1 to 65536 bins");
        if ((uint64_t)npts * xt_cells(&xt_spec) > (1ull << 24)) die("--xtab: too many cells");
        red_ci.kind = PRACH_G_XTAB; red_ci.spec = &xt_spec; red_ci.path = xt_path; red_ci.text_cap = 64 * (xt_cells(&xt_spec) + 1) + 1; /* (a line: the label, two edges, a count) */
    }
    /* --census: the NOMA menu's axes as given, the defaults of a field where width or bins are left out */
    prach_xtab_spec nc_spec = {0, 0, 0, 0, 0, 0, 0, npts, {0, 0}};
    if (nc_path) {
        nc_spec.who = strcmp(nc_who, "served") == 0 ? PRACH_NOMA_SERVED : strcmp(nc_who, "pending") == 0 ? PRACH_NOMA_PENDING : strcmp(nc_who, "dropped") == 0 ? PRACH_NOMA_DROPPED
                      : strcmp(nc_who, "arrived") == 0 ? (PRACH_NOMA_SERVED | PRACH_NOMA_PENDING | PRACH_NOMA_DROPPED)
                      : strcmp(nc_who, "all") == 0 ? (PRACH_NOMA_SERVED | PRACH_NOMA_PENDING | PRACH_NOMA_DROPPED | PRACH_NOMA_IDLE) : 0;
        if (!nc_spec.who) die("--census-who served|pending|dropped|arrived|all");
        if (!noma_axis(nc_rows, prach_max_time(&base), &nc_spec.row_field, &nc_spec.row_width, &nc_spec.row_bins)) die("--census-rows FIELD[:WIDTH[:BINS]]: a field of the NOMA menu, a width of at least 1, 1 to 65536 bins");
        if (!noma_axis(nc_cols, prach_max_time(&base), &nc_spec.col_field, &nc_spec.col_width, &nc_spec.col_bins)) die("--census-cols FIELD[:WIDTH[:BINS]]: a field of the NOMA menu, a width of at least 1, 1 to 65536 bins");
        if ((uint64_t)npts * xt_cells(&nc_spec) > (1ull << 24)) die("--census: too many cells");
        red_ci.kind = PRACH_G_NOMA_CENSUS; red_ci.spec = &nc_spec; red_ci.path = nc_path; red_ci.text_cap = 64 * (xt_cells(&nc_spec) + 1) + 1; /* (a line: the label, two edges, a count) */
    }
    if (ci_path) { /* --ci: the rows of the whole grid, filled by the workers */
        red_ci.sm = &ci_spec;
        red_ci.sm_rows = (prach_trial_summary *)mmap(NULL, sizeof(prach_trial_summary) * (size_t)ntr, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (red_ci.sm_rows == MAP_FAILED) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int q = 0; q < ntr; q++) red_ci.sm_rows[q].status = PRACH_ERR_INTERNAL; /* (a row no worker wrote counts nowhere) */
    }
    if (nci_path) { /* --census-ci: the rows of the whole grid, filled by the workers */
        nci_spec.who = noma_who(nci_who, 0);
        if (!nci_spec.who) die("--census-ci-who served|pending|dropped|arrived|all");
        red_ci.nsm = &nci_spec;
        red_ci.nsm_rows = (prach_noma_trial_summary *)mmap(NULL, sizeof(prach_noma_trial_summary) * (size_t)ntr, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (red_ci.nsm_rows == MAP_FAILED) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int q = 0; q < ntr; q++) red_ci.nsm_rows[q].status = PRACH_ERR_INTERNAL; /* (a row no worker wrote counts nowhere) */
    }
    if (npk_path) { /* --census-pick: --pick's mappings and lines, over the NOMA menu */
        npk_spec.who = noma_who(npk_who, 1);
        if (!npk_spec.who) die("--census-pick-who served|pending|dropped|arrived|idle|all");
        pk_spec = npk_spec;
        pk_path = npk_path;
        red_ci.pk_noma = 1;
    }
    if (pk_path) { /* --pick: the headers and rows of the whole grid, filled by the workers */
        if (!red_ci.pk_noma) pk_spec.who = strcmp(pk_who, "served") == 0 ? PRACH_XTAB_SERVED : strcmp(pk_who, "unserved") == 0 ? PRACH_XTAB_UNSERVED : strcmp(pk_who, "idle") == 0 ? PRACH_XTAB_IDLE
                      : strcmp(pk_who, "arrived") == 0 ? (PRACH_XTAB_SERVED | PRACH_XTAB_UNSERVED) : strcmp(pk_who, "all") == 0 ? (PRACH_XTAB_SERVED | PRACH_XTAB_UNSERVED | PRACH_XTAB_IDLE) : 0;
        if (!pk_spec.who) die("--pick-who served|unserved|arrived|idle|all");
        if ((uint64_t)ntr * (uint64_t)pk_spec.k > (1ull << 22)) die(red_ci.pk_noma ? "--census-pick: too many rows" : "--pick: too many rows");
        red_ci.pk = &pk_spec;
        red_ci.pk_hdr = (prach_pick *)mmap(NULL, sizeof(prach_pick) * (size_t)ntr, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        red_ci.pk_rows = (prach_pick_row *)mmap(NULL, sizeof(prach_pick_row) * (size_t)ntr * (size_t)pk_spec.k, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (red_ci.pk_hdr == MAP_FAILED || red_ci.pk_rows == MAP_FAILED) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int q = 0; q < ntr; q++) { red_ci.pk_hdr[q].status = PRACH_ERR_INTERNAL; red_ci.pk_hdr[q].nUE = cfgs[q].nUE; red_ci.pk_hdr[q].threshold = -1; } /* (a trial no worker wrote) */
    }
    const reduction *const red = &red_ci;
    char *red_blocks = NULL;
    if (red_on(red)) {
        red_blocks = (char *)mmap(NULL, red_block_bytes(red) * (size_t)gpus, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0); /* (zero-filled) */
        if (red_blocks == MAP_FAILED) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int w = 0; w < gpus; w++) red_init_block(red, red_blocks + red_block_bytes(red) * (size_t)w);
    }
#define RED_BLOCK(w) (red_on(red) ? red_blocks + red_block_bytes(red) * (size_t)(w) : NULL)

    if (gpus == 1) {
        int rcw = run_worker(devs[0], cfgs, widx[0], wn[0], res, lat, want_logs, outdir, glibc, npts, red, RED_BLOCK(0));
        if (rcw) return rcw;
    } else {
        /* one child per device, forked BEFORE this process touches HIP (a forked copy of an initialised runtime is not usable) */
        pid_t *pid = (pid_t *)calloc((size_t)gpus, sizeof(pid_t));
        if (!pid) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int w = 0; w < gpus; w++) {
            pid[w] = fork();
            if (pid[w] < 0) { perror("prach_sim: fork"); return 2; }
            if (pid[w] == 0) _exit(run_worker(devs[w], cfgs, widx[w], wn[w], res, lat, want_logs, outdir, glibc, npts, red, RED_BLOCK(w)));
        }
        int bad = 0;
        for (int w = 0; w < gpus; w++) {
            int st = 0;
            if (waitpid(pid[w], &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) {
                fprintf(stderr, "prach_sim: the worker of device %d failed\n", devs[w]);
                bad = 1;
            }
        }
        free(pid);
        if (bad) return 2;
    }

    if (red_on(red)) { /* worker 0's block takes the others'; one group per sweep point, labelled nUE */
        for (int w = 1; w < gpus; w++) red_merge_block(red, RED_BLOCK(0), RED_BLOCK(w));
        FILE *fp = fopen(red->path, "wb");
        if (!fp) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_IO)); return 2; }
        char *out = (char *)malloc(red->text_cap);
        if (!out) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int k = 0; k < npts; k++) {
            char label[16];
            snprintf(label, sizeof label, "%d", sweep_lo + k * sweep_step);
            const size_t n = red_format_group(red, RED_BLOCK(0), k, label, out, red->text_cap);
            if (n >= red->text_cap) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_INTERNAL)); return 2; }
            fwrite(out, 1, n, fp);
        }
        free(out);
        fclose(fp);
    }

    if (ci_path) { /* statistics over the seeds of every sweep point, from the rows in trial order: the same whatever the number of workers */
        const int nm = 5 + 3 * ci_spec.nq;
        int32_t *grp = (int32_t *)malloc(sizeof(int32_t) * (size_t)ntr);
        prach_stat *st = (prach_stat *)malloc(sizeof(prach_stat) * (size_t)npts * (size_t)nm);
        if (!grp || !st) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int q = 0; q < ntr; q++) grp[q] = q % npts;
        const int rcs = prach_summary_stats(&ci_spec, red->sm_rows, ntr, grp, npts, st);
        if (rcs != PRACH_OK) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(rcs)); return 2; }
        FILE *fp = fopen(ci_path, "wb");
        if (!fp) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_IO)); return 2; }
        char out[8192]; /* 29 lines at most: a label of at most 10 digits, a name of at most 14 characters, seven numbers of at most 16 */
        for (int k = 0; k < npts; k++) {
            char label[16];
            snprintf(label, sizeof label, "%d", sweep_lo + k * sweep_step);
            const size_t n = prach_summary_format_csv(&ci_spec, st + (size_t)k * (size_t)nm, label, out, sizeof out);
            if (n >= sizeof out) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_INTERNAL)); return 2; }
            fwrite(out, 1, n, fp);
        }
        fclose(fp);
        free(grp); free(st);
    }

    if (nci_path) { /* statistics over the seeds of every sweep point, from the rows in trial order: the same whatever the number of workers */
        const int nm = 4 + nci_spec.nfields * (1 + nci_spec.nq);
        int32_t *grp = (int32_t *)malloc(sizeof(int32_t) * (size_t)ntr);
        prach_stat *st = (prach_stat *)malloc(sizeof(prach_stat) * (size_t)npts * (size_t)nm);
        if (!grp || !st) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int q = 0; q < ntr; q++) grp[q] = q % npts;
        const int rcs = prach_noma_summary_stats(&nci_spec, red->nsm_rows, ntr, grp, npts, st);
        if (rcs != PRACH_OK) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(rcs)); return 2; }
        FILE *fp = fopen(nci_path, "wb");
        if (!fp) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_IO)); return 2; }
        char out[8192]; /* 40 lines at most: a label of at most 10 digits, a name of at most 16 characters, seven numbers of at most 16 */
        for (int k = 0; k < npts; k++) {
            char label[16];
            snprintf(label, sizeof label, "%d", sweep_lo + k * sweep_step);
            const size_t n = prach_noma_summary_format_csv(&nci_spec, st + (size_t)k * (size_t)nm, label, out, sizeof out);
            if (n >= sizeof out) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_INTERNAL)); return 2; }
            fwrite(out, 1, n, fp);
        }
        fclose(fp);
        free(grp); free(st);
    }

    if (pk_path) { /* every trial of the grid in trial order, labelled nUE: the same whatever the number of workers */
        FILE *fp = fopen(pk_path, "wb");
        if (!fp) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_IO)); return 2; }
        const size_t cap = 512 * ((size_t)pk_spec.k + 1) + 1; /* (a line is shorter than the 512 bytes of the formatter's own line buffer) */
        char *out = (char *)malloc(cap);
        if (!out) { fprintf(stderr, "prach_sim: out of memory\n"); return 2; }
        for (int q = 0; q < ntr; q++) {
            char label[16];
            snprintf(label, sizeof label, "%d", cfgs[q].nUE);
            const size_t n = (red->pk_noma ? prach_noma_pick_format_csv : prach_pick_format_csv)(&pk_spec, &red->pk_hdr[q], red->pk_rows + (size_t)q * (size_t)pk_spec.k, label, q,
                                                                                                 cfgs[q].seed, out, cap);
            if (n == 0 || n >= cap) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_INTERNAL)); return 2; }
            fwrite(out, 1, n, fp);
        }
        free(out);
        fclose(fp);
    }

    /* the parent prints in the reference's order and merges */
    char text[4096];
    if (variant == PRACH_VARIANT_NOMA_C) { /* NOMA.c main: no banner, one line per trial, "Done" per seed */
        char line[256], path[1024];
        for (int s_ = 0; s_ < randomMax; s_++) {
            for (int k = 0; k < npts; k++) {
                const int q = s_ * npts + k;
                prach_format_noma_line(&cfgs[q], &res[q], line, sizeof line);
                fputs(line, stdout);
                snprintf(path, sizeof path, "%s/TestResults/Sector_%d_Result.txt", outdir, cfgs[q].nUE); /* NOMA.c:603-605 */
                FILE *fp = fopen(path, "a");
                if (!fp) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_IO)); return 2; }
                fputs(line, fp);
                fclose(fp);
            }
            printf("Done\n"); /* NOMA.c:716 */
        }
        return 0;
    }
    for (int q = 0; q < ntr; q++) {
        prach_format_stdout(&cfgs[q], &res[q], lat[q], text, sizeof text);
        fputs(text, stdout);
    }
    if (csv_path) { /* one row per sweep point: mean over the seeds in seed order (AveragePerformance.py:8-24), np.around(., 3), csv.writer's float repr and CRLF */
        FILE *fp = fopen(csv_path, "wb");
        if (!fp) { fprintf(stderr, "prach_sim: %s\n", prach_strerror(PRACH_ERR_IO)); return 2; }
        for (int k = 0; k < npts; k++) {
            double acc[6] = {0, 0, 0, 0, 0, 0};
            for (int s_ = 0; s_ < randomMax; s_++) {
                prach_format_results(&cfgs[s_ * npts + k], &res[s_ * npts + k], lat[s_ * npts + k], text, sizeof text);
                prach_results_csv_accumulate(acc, text);
            }
            const size_t n = prach_results_csv_row(acc, randomMax, text, sizeof text);
            fwrite(text, 1, n, fp);
        }
        fclose(fp);
    }
    for (int w = 0; w < gpus; w++) free(widx[w]);
    free(widx); free(wn); free(wload); free(cfgs);
    return 0;
}
