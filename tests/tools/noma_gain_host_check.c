/* noma_gain_host_check.c — drives the host functions of NOMA.c's near-far profile (include/prach.h: prach_noma_gain_level, _levels, _accumulate_levels,
 * _accumulate_logs, _merge, _format_csv and the row of the grouped table behind them) with every buffer allocated at its exact size: the level at its edge
 * values, a small trial's levels, the definition on records of every class at the smallest and the largest bin count, the lowest and the highest lower edge,
 * a merge with an empty group on either side, the CSV into a buffer of the exact length and one byte short.  tests/test_noma_gain_cpu.py compiles it together
 * with csrc/prach_host.c under -fsanitize=address,undefined on the CPU and asserts the exit status: 0, or the line number of the first check that failed
 * (modulo 250, plus 1). */
#include "../../5g-nr-randomaccess_amd/csrc/prach_grouped.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "noma_gain_host_check: line %d: %s\n", __LINE__, #x); exit(__LINE__ % 250 + 1); } } while (0)

typedef struct profile { prach_noma_gain *g; uint64_t *series[6]; } profile;
static profile make_profile(int bins) {
    profile p;
    p.g = (prach_noma_gain *)calloc(1, sizeof(prach_noma_gain));
    CHECK(p.g);
    for (int q = 0; q < 6; q++) { p.series[q] = (uint64_t *)calloc(6 * (size_t)bins, 8); CHECK(p.series[q]); }
    return p;
}
static void free_profile(profile *p) {
    free(p->g);
    for (int q = 0; q < 6; q++) free(p->series[q]);
}
static uint64_t sum_of(const uint64_t *a, int n) { uint64_t s = 0; for (int i = 0; i < n; i++) s += a[i]; return s; }

int main(void) {
    /* the level */
    CHECK(prach_noma_gain_level(0.0) == 0 && prach_noma_gain_level(-0.0005) == -1 && prach_noma_gain_level(0.0005) == 0 && prach_noma_gain_level(-5.0) == -5000);
    CHECK(prach_noma_gain_level(NAN) == PRACH_NOMA_GAIN_NO_LEVEL && prach_noma_gain_level(INFINITY) == PRACH_NOMA_GAIN_NO_LEVEL && prach_noma_gain_level(-INFINITY) == PRACH_NOMA_GAIN_NO_LEVEL);
    CHECK(prach_noma_gain_level(1073741.824) == PRACH_NOMA_GAIN_NO_LEVEL || prach_noma_gain_level(1073741.824) == 1073741823); /* 2^30 / 1000, as it rounds */
    CHECK(prach_noma_gain_level(1e308) == PRACH_NOMA_GAIN_NO_LEVEL && prach_noma_gain_level(-1e308) == PRACH_NOMA_GAIN_NO_LEVEL && prach_noma_gain_level(1073741.0) == 1073741000);

    /* a small trial's levels and records of every class */
    enum { N = 97 };
    prach_cfg cfg;
    prach_cfg_defaults(&cfg, PRACH_VARIANT_NOMA_C);
    cfg.nUE = N; cfg.rng_mode = PRACH_RNG_PHILOX; cfg.seed = 3;
    CHECK(prach_cfg_validate(&cfg) == PRACH_OK);
    int32_t *level = (int32_t *)malloc(4 * N);
    prach_ue_log *ue = (prach_ue_log *)calloc(N, sizeof(prach_ue_log));
    CHECK(level && ue);
    CHECK(prach_noma_gain_levels(&cfg, level) == PRACH_OK && prach_noma_gain_levels(NULL, level) == PRACH_ERR_ARG && prach_noma_gain_levels(&cfg, NULL) == PRACH_ERR_ARG);
    for (int i = 0; i < N; i++) CHECK(level[i] > -16200 && level[i] < -3300);
    for (int i = 0; i < N; i++) {
        ue[i].idx = i;
        ue[i].preambleChange = i % 11 == 0 ? -1 : i % 13 == 0 ? 6 : i % 6; /* idle; a sector outside 0..5; a sector */
        ue[i].msg4Flag = i % 3 == 0;
        ue[i].failCount = i % 5 == 0;
        ue[i].txTime = i % 17 == 0 ? -20 : 10000;                       /* a served UE that completes before it arrives; behind every arrival */
        ue[i].timer = i % 19 == 0 ? -1 : 7;
        ue[i].preambleTxCounter = i % 23 == 0 ? -1 : 2;
        ue[i].active = 1;
    }
    level[5] = PRACH_NOMA_GAIN_NO_LEVEL; level[6] = INT32_MAX; level[7] = INT32_MIN + 1;

    static const prach_noma_gain_spec specs[] = {{1, 1, -16200, 1, 0}, {PRACH_NOMA_GAIN_MAX_BINS, 4, -16384, 1, 0}, {65, 200, -16200, 1, 0}, {3, INT32_MAX, INT32_MIN, 1, 0},
                                                 {2, 1 << 20, INT32_MAX - 5, 1, 0}};
    for (size_t k = 0; k < sizeof specs / sizeof specs[0]; k++) {
        const prach_noma_gain_spec *s = &specs[k];
        profile a = make_profile(s->bins), b = make_profile(s->bins), e = make_profile(s->bins);
        CHECK(prach_noma_gain_accumulate_levels(s, &cfg, 10000, ue, N, level, a.g, a.series) == PRACH_OK);
        CHECK(a.g->trials == 1 && a.g->ues == N && a.g->idle + a.g->served + a.g->dropped + a.g->pending == N);
        CHECK(sum_of(a.series[0], 6 * s->bins) + a.g->below + a.g->above + a.g->undefined == a.g->served + a.g->dropped + a.g->pending);
        CHECK(sum_of(a.series[0], 6 * s->bins) + a.g->below + a.g->above == a.g->defined && a.g->undefined > 0 && a.g->level_max == INT32_MAX && a.g->neg_level_max == INT32_MAX);
        CHECK(prach_noma_gain_accumulate_logs(s, &cfg, 10000, ue, N, b.g, b.series) == PRACH_OK && b.g->ues == N && b.g->level_max < -3300 && b.g->neg_level_max < 16200);
        /* refusals touch nothing */
        const prach_noma_gain before = *b.g;
        prach_cfg other = cfg;
        other.rng_mode = PRACH_RNG_GLIBC;
        CHECK(prach_noma_gain_accumulate_logs(s, &other, 10000, ue, N, b.g, b.series) == PRACH_ERR_UNSUPPORTED);
        CHECK(prach_noma_gain_accumulate_levels(s, &cfg, 10000, ue, N - 1, level, b.g, b.series) == PRACH_ERR_ARG);
        CHECK(prach_noma_gain_accumulate_levels(s, &cfg, 10000, ue, N, NULL, b.g, b.series) == PRACH_ERR_ARG && memcmp(&before, b.g, sizeof before) == 0);
        /* merge: an empty group on either side never wins a maximum; garbage in its maxima is not read */
        e.g->level_max = 123456; e.g->neg_level_max = 654321;
        const prach_noma_gain b0 = *b.g;
        prach_noma_gain_merge(s, b.g, b.series, e.g, (const uint64_t *const *)e.series);
        CHECK(memcmp(&b0, b.g, sizeof b0) == 0);
        prach_noma_gain_merge(s, e.g, e.series, b.g, (const uint64_t *const *)b.series);
        CHECK(memcmp(&b0, e.g, sizeof b0) == 0 && sum_of(e.series[0], 6 * s->bins) == sum_of(b.series[0], 6 * s->bins));
        prach_noma_gain_merge(s, a.g, a.series, b.g, (const uint64_t *const *)b.series);
        CHECK(a.g->trials == 2 && a.g->level_max == INT32_MAX && a.g->defined > b.g->defined);
        /* CSV: the length, then a buffer of exactly that length plus the terminator, then one byte short */
        const size_t need = prach_noma_gain_format_csv(s, a.g, (const uint64_t *const *)a.series, "p", NULL, 0);
        CHECK(need > 0);
        char *buf = (char *)malloc(need + 1), *shortbuf = (char *)malloc(need);
        CHECK(buf && shortbuf);
        CHECK(prach_noma_gain_format_csv(s, a.g, (const uint64_t *const *)a.series, "p", buf, need + 1) == need && strlen(buf) == need && buf[need - 1] == '\n');
        CHECK(prach_noma_gain_format_csv(s, a.g, (const uint64_t *const *)a.series, "p", shortbuf, need) == need && shortbuf[0] == 0);
        CHECK(prach_noma_gain_format_csv(s, NULL, (const uint64_t *const *)a.series, "p", buf, need + 1) == 0);
        free(buf); free(shortbuf);
        free_profile(&a); free_profile(&b); free_profile(&e);
    }
    /* bad specs are refused by every function */
    {
        static const prach_noma_gain_spec bad[] = {{0, 1, 0, 1, 0}, {PRACH_NOMA_GAIN_MAX_BINS + 1, 1, 0, 1, 0}, {4, 0, 0, 1, 0}, {4, -1, 0, 1, 0}};
        profile a = make_profile(4);
        for (size_t k = 0; k < sizeof bad / sizeof bad[0]; k++) {
            CHECK(prach_noma_gain_accumulate_levels(&bad[k], &cfg, 10000, ue, N, level, a.g, a.series) == PRACH_ERR_ARG);
            CHECK(prach_noma_gain_format_csv(&bad[k], a.g, (const uint64_t *const *)a.series, "p", NULL, 0) == 0 && a.g->trials == 0);
        }
        free_profile(&a);
    }
    /* the row of the grouped table */
    const prach_grouped_row *row = prach_internal_grouped_row(PRACH_G_NOMA_GAIN);
    CHECK(row && row->spec_bytes == sizeof(prach_noma_gain_spec) && row->group_bytes == sizeof(prach_noma_gain) && row->counters == 14 && row->maxima == 2);
    CHECK(row->guard == (int)(offsetof(prach_noma_gain, defined) / 8) && row->trials == PRACH_G_TRIALS_NOMA_C_PHILOX && row->reserved_words == 1);
    CHECK(prach_internal_grouped_row(PRACH_G_KINDS) == NULL && prach_internal_grouped_row(PRACH_G_MORE_END) == NULL && prach_internal_grouped_row(PRACH_G_MORE - 1) == NULL);
    free(level); free(ue);
    printf("noma_gain_host_check: ok\n");
    return 0;
}
