/* grouped_host_check.c — drives the generic shape, merge and CSV functions of the grouped kinds (csrc/prach_grouped.h) over all eight kinds at the smallest
 * shapes that can still go wrong, with every buffer allocated at its exact size.  tests/test_grouped_cpu.py compiles it together with csrc/prach_host.c under
 * -fsanitize=address,undefined on the CPU and asserts the exit status: 0, or the line number of the first check that failed (modulo 250, plus 1). */
#include "../../5g-nr-randomaccess_amd/csrc/prach_grouped.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "grouped_host_check: line %d: %s\n", __LINE__, #x); exit(__LINE__ % 250 + 1); } } while (0)

typedef union any_spec {
    prach_dist_spec dist;
    prach_timeline_spec timeline;
    prach_sojourn_spec sojourn;
    prach_trace_spec trace;
    prach_xtab_spec xtab;
    prach_noma_trace_spec noma_trace;
    prach_noma_timeline_spec noma_timeline;
} any_spec;

/* variant 0: bins 1 (sojourn 2 x 3, census axes of 1 and 2 bins); variant 1: bins 3 (sojourn 3 x 2, census axes of 2 and 1 bins) */
static void make_spec(int kind, int variant, int ngroups, any_spec *s) {
    const int bins = variant ? 3 : 1;
    memset(s, 0, sizeof *s);
    switch (kind) {
    case PRACH_G_DIST: s->dist = (prach_dist_spec){bins, 2, ngroups, 0}; break;
    case PRACH_G_TIMELINE: s->timeline = (prach_timeline_spec){bins, 5, ngroups, 0}; break;
    case PRACH_G_SOJOURN: s->sojourn = (prach_sojourn_spec){variant ? 3 : 2, 500, variant ? 2 : 3, 5, ngroups, 0}; break;
    case PRACH_G_TRACE: s->trace = (prach_trace_spec){bins, 5, ngroups, 0}; break;
    case PRACH_G_XTAB: s->xtab = (prach_xtab_spec){PRACH_XTAB_SERVED | PRACH_XTAB_UNSERVED, PRACH_XTAB_ARRIVAL, 500, variant ? 2 : 1, PRACH_XTAB_STATE, 1, variant ? 1 : 2, ngroups, {0, 0}}; break;
    case PRACH_G_NOMA_CENSUS: s->xtab = (prach_xtab_spec){PRACH_NOMA_SERVED, PRACH_NOMA_ARRIVAL, 500, variant ? 2 : 1, PRACH_NOMA_SECTOR, 1, variant ? 1 : 2, ngroups, {0, 0}}; break;
    case PRACH_G_NOMA_TRACE: s->noma_trace = (prach_noma_trace_spec){bins, 5, ngroups, 0}; break;
    default: s->noma_timeline = (prach_noma_timeline_spec){bins, 5, ngroups, 0}; break;
    }
}

static size_t expected_words(int kind, int variant, int q) {
    const size_t bins = variant ? 3 : 1;
    switch (kind) {
    case PRACH_G_DIST: return q == 0 ? bins : PRACH_DIST_PTC_BINS;
    case PRACH_G_SOJOURN: return q == 0 ? 6 : (variant ? 3 : 2);
    case PRACH_G_XTAB: case PRACH_G_NOMA_CENSUS: return 6; /* (1 + 1) * (2 + 1) */
    case PRACH_G_NOMA_TRACE: case PRACH_G_NOMA_TIMELINE: return 6 * bins;
    default: return bins;
    }
}
static const int expected_arrays[PRACH_G_KINDS] = {2, 5, 3, 4, 1, 1, 6, 6};

/* a group of exact size: struct and arrays of their own allocations, filled from `seed` (0: an empty group, whose maxima hold garbage under a zero guard) */
typedef struct group { uint64_t *head; uint64_t *arrays[PRACH_G_MAX_ARRAYS]; } group;
static group make_group(const prach_grouped_row *k, int narrays, const size_t *words, uint64_t seed) {
    group g;
    g.head = (uint64_t *)malloc(k->group_bytes);
    CHECK(g.head);
    for (int c = 0; c < k->counters; c++) g.head[c] = seed ? seed * 1000 + (uint64_t)c + 1 : 0;
    for (int m = 0; m < k->maxima; m++) ((int64_t *)g.head)[k->counters + m] = seed ? (int64_t)(seed * 7) + m : 123456 + m;
    for (int q = 0; q < PRACH_G_MAX_ARRAYS; q++) g.arrays[q] = NULL;
    for (int q = 0; q < narrays; q++) {
        g.arrays[q] = (uint64_t *)malloc(8 * words[q]);
        CHECK(g.arrays[q]);
        for (size_t i = 0; i < words[q]; i++) g.arrays[q][i] = seed ? seed * 100 + (uint64_t)q * 10 + i % 7 : 0;
    }
    return g;
}
static void free_group(group *g) {
    free(g->head);
    for (int q = 0; q < PRACH_G_MAX_ARRAYS; q++) free(g->arrays[q]);
}

static void check_kind(int kind, int variant, int ngroups) {
    const prach_grouped_row *k = prach_internal_grouped_row(kind);
    CHECK(k && 8 * (size_t)(k->counters + k->maxima) == k->group_bytes && k->guard >= 0 && k->guard < k->counters);
    any_spec spec;
    make_spec(kind, variant, ngroups, &spec);
    CHECK(k->spec_bytes <= sizeof spec && *(const int32_t *)((const char *)&spec + k->ngroups_at) == ngroups);
    size_t words[PRACH_G_MAX_ARRAYS];
    const int na = prach_internal_grouped_shape(kind, &spec, words);
    CHECK(na == expected_arrays[kind]);
    for (int q = 0; q < na; q++) CHECK(words[q] == expected_words(kind, variant, q));

    /* merge: the four combinations of an empty and a filled `into` and `from` */
    for (int combo = 0; combo < 4; combo++) {
        const uint64_t sa = combo & 1 ? 3 : 0, sb = combo & 2 ? 5 : 0;
        group a = make_group(k, na, words, sa), b = make_group(k, na, words, sb), b0 = make_group(k, na, words, sb);
        prach_internal_grouped_merge(kind, &spec, a.head, a.arrays, b.head, (const uint64_t *const *)b.arrays);
        for (int c = 0; c < k->counters; c++) CHECK(a.head[c] == (sa ? sa * 1000 + (uint64_t)c + 1 : 0) + (sb ? sb * 1000 + (uint64_t)c + 1 : 0));
        for (int m = 0; m < k->maxima; m++) {
            const int64_t x = sa ? (int64_t)(sa * 7) + m : -1, y = sb ? (int64_t)(sb * 7) + m : -1;
            CHECK(((int64_t *)a.head)[k->counters + m] == (x > y ? x : y));
        }
        for (int q = 0; q < na; q++)
            for (size_t i = 0; i < words[q]; i++) CHECK(a.arrays[q][i] == (sa ? sa * 100 + (uint64_t)q * 10 + i % 7 : 0) + (sb ? sb * 100 + (uint64_t)q * 10 + i % 7 : 0));
        CHECK(memcmp(b.head, b0.head, k->group_bytes) == 0); /* `from` is only read */
        free_group(&a); free_group(&b); free_group(&b0);
    }

    /* a bad spec or a missing pointer: merge touches nothing, the formatter returns 0 */
    {
        group a = make_group(k, na, words, 3), a0 = make_group(k, na, words, 3), b = make_group(k, na, words, 5);
        any_spec bad = spec;
        *(int32_t *)&bad = 0; /* the first word of every spec is a count of at least 1 (xtab: `who`, not empty) */
        size_t w2[PRACH_G_MAX_ARRAYS];
        CHECK(prach_internal_grouped_shape(kind, &bad, w2) == 0 && prach_internal_grouped_shape(kind, NULL, w2) == 0 && prach_internal_grouped_shape(PRACH_G_KINDS, &spec, w2) == 0);
        uint64_t *holed[PRACH_G_MAX_ARRAYS];
        memcpy(holed, b.arrays, sizeof holed);
        holed[na - 1] = NULL;
        prach_internal_grouped_merge(kind, &bad, a.head, a.arrays, b.head, (const uint64_t *const *)b.arrays);
        prach_internal_grouped_merge(kind, NULL, a.head, a.arrays, b.head, (const uint64_t *const *)b.arrays);
        prach_internal_grouped_merge(kind, &spec, NULL, a.arrays, b.head, (const uint64_t *const *)b.arrays);
        prach_internal_grouped_merge(kind, &spec, a.head, NULL, b.head, (const uint64_t *const *)b.arrays);
        prach_internal_grouped_merge(kind, &spec, a.head, a.arrays, NULL, (const uint64_t *const *)b.arrays);
        prach_internal_grouped_merge(kind, &spec, a.head, a.arrays, b.head, NULL);
        prach_internal_grouped_merge(kind, &spec, a.head, a.arrays, b.head, (const uint64_t *const *)holed);
        prach_internal_grouped_merge(kind, &spec, a.head, holed, b.head, (const uint64_t *const *)b.arrays);
        CHECK(memcmp(a.head, a0.head, k->group_bytes) == 0);
        for (int q = 0; q < na; q++) CHECK(memcmp(a.arrays[q], a0.arrays[q], 8 * words[q]) == 0);
        char buf[64];
        CHECK(prach_internal_grouped_format_csv(kind, &bad, a.head, (const uint64_t *const *)a.arrays, "x", buf, sizeof buf) == 0);
        CHECK(prach_internal_grouped_format_csv(kind, &spec, NULL, (const uint64_t *const *)a.arrays, "x", buf, sizeof buf) == 0);
        CHECK(prach_internal_grouped_format_csv(kind, &spec, a.head, (const uint64_t *const *)holed, "x", buf, sizeof buf) == 0);
        CHECK(prach_internal_grouped_format_csv(kind, &spec, a.head, (const uint64_t *const *)a.arrays, NULL, buf, sizeof buf) == 0);
        free_group(&a); free_group(&a0); free_group(&b);
    }

    /* CSV: the size-only call, a buffer that fits exactly, a buffer one byte too small */
    {
        group a = make_group(k, na, words, 3);
        const uint64_t *const *arr = (const uint64_t *const *)a.arrays;
        const size_t need = prach_internal_grouped_format_csv(kind, &spec, a.head, arr, "10000", NULL, 0);
        CHECK(need > 0);
        char *fits = (char *)malloc(need + 1), *tight = (char *)malloc(need);
        CHECK(fits && tight);
        memset(tight, 'x', need);
        CHECK(prach_internal_grouped_format_csv(kind, &spec, a.head, arr, "10000", fits, need + 1) == need && strlen(fits) == need && fits[need - 1] == '\n');
        CHECK(strncmp(fits, "10000,", 6) == 0);
        CHECK(prach_internal_grouped_format_csv(kind, &spec, a.head, arr, "10000", tight, need) == need && tight[0] == 0); /* (nothing partial is left behind as a string) */
        free(fits); free(tight);
        free_group(&a);
    }
}

int main(void) {
    CHECK(prach_internal_grouped_row(-1) == NULL && prach_internal_grouped_row(PRACH_G_KINDS) == NULL);
    for (int kind = 0; kind < PRACH_G_KINDS; kind++)
        for (int variant = 0; variant < 2; variant++)
            for (int ngroups = 1; ngroups <= 2; ngroups++) check_kind(kind, variant, ngroups);
    printf("grouped_host_check: %d kinds ok\n", PRACH_G_KINDS);
    return 0;
}
