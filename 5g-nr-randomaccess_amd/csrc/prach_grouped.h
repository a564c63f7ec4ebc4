/* prach_grouped.h — the host-side row of every GROUPED reduction (one struct and a few uint64 arrays per trial group): what prach_host.c (shape, merge, CSV),
 * prach_engine.hip (the one refusal sequence in front of run_trials_impl) and prach_cli.c (the block of groups of a worker) know about a kind.  Internal:
 * include/prach.h states the 24 public functions, which are wrappers that gather their pointers into an array and call the generic function.
 *
 * A new grouped kind is an enumerator here (of the second block: PRACH_G_MORE), a row of GROUPED_MORE in prach_host.c (with its shape function and its CSV
 * lines) and an entry of the engine's GROUPED_RED_MORE; the generic functions and the CLI's block code do not change. */
#ifndef PRACH_GROUPED_H
#define PRACH_GROUPED_H

#include "../../include/prach.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PRACH_G_DIST, PRACH_G_TIMELINE, PRACH_G_SOJOURN, PRACH_G_TRACE, PRACH_G_XTAB, PRACH_G_NOMA_CENSUS, PRACH_G_NOMA_TRACE, PRACH_G_NOMA_TIMELINE, PRACH_G_KINDS };
/* The kinds behind the first eight: PRACH_G_KINDS is the size of the first block of GROUPED and stays what the checks of that block know it as; a later kind
 * counts from PRACH_G_MORE in a second block of the same rows.  Every generic function takes the kinds of both blocks. */
enum { PRACH_G_MORE = 16, PRACH_G_NOMA_GAIN = PRACH_G_MORE, PRACH_G_MORE_END };
#define PRACH_G_MAX_ARRAYS 6
/* the trials a kind's device call takes: any; every program but NOMA.c; NOMA.c with Philox only */
enum { PRACH_G_TRIALS_ANY, PRACH_G_TRIALS_NOT_NOMA_C, PRACH_G_TRIALS_NOMA_C_PHILOX };

typedef struct prach_grouped_row {
    size_t spec_bytes, group_bytes;    /* sizeof the kind's prach_*_spec and of its per-group struct */
    int counters, maxima, guard;       /* the struct: `counters` uint64_t that add up, then `maxima` int64_t that hold something only if counter `guard` is non-zero */
    /* words per group of every array, in the order of the C ABI; returns their number, 0 for a NULL spec or one whose ranges are out of bounds.  The host-side
       judge of a spec: it does not look at ngroups, nor at reserved words unless the kind's merge and CSV always did */
    int (*shape)(const void *spec, size_t words[PRACH_G_MAX_ARRAYS]);
    size_t ngroups_at, reserved_at;    /* byte offsets of the spec's int32_t ngroups and of its first reserved word */
    int reserved_words;
    int trials;                        /* PRACH_G_TRIALS_* */
    /* the CSV lines of one group: spec, group and arrays are valid (prach_internal_grouped_format_csv has judged them); returns the text's size, 0 on an overlong line */
    size_t (*format)(const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap);
} prach_grouped_row;

const prach_grouped_row *prach_internal_grouped_row(int kind); /* NULL: no such kind */
int prach_internal_grouped_shape(int kind, const void *spec, size_t words[PRACH_G_MAX_ARRAYS]);
/* adds group `from` to group `into`; touches nothing on a bad spec or a NULL pointer */
void prach_internal_grouped_merge(int kind, const void *spec, void *into, uint64_t *const into_arrays[], const void *from, const uint64_t *const from_arrays[]);
/* the CSV text of one group, as every prach_*_format_csv returns it; 0 on a bad spec or a NULL pointer */
size_t prach_internal_grouped_format_csv(int kind, const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap);
/* prach_run_trials plus the kind's reduction (prach_engine.hip): groups[ngroups] and arrays[q][ngroups * words[q]] are the caller's */
int prach_internal_grouped_run(int kind, prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const void *spec,
                               const int32_t *group, void *groups, uint64_t *const arrays[]);

#ifdef __cplusplus
}
#endif
#endif
