/* prach_host.c — host-side half of the C ABI that needs no device: parameter defaults and
 * validation, the deterministic arrival schedule, the glibc rand() stream, and the reference's
 * text surfaces (stdout block, Results.txt, Logs.txt).  Plain C like the reference.
 *
 * Reference lines are cited per function; nothing here is copied from the reference — the
 * formats are reproduced because the drop-in boundary of this project IS those files
 * (SURVEY.md §8b).
 */
#define _GNU_SOURCE
#include "prach_grouped.h"

#include <errno.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

/* Beta.c:47-57 (BETA_C) / WithNOMA:70-88 (WITHNOMA_C): the hard-coded / default parameters */
void prach_cfg_defaults(prach_cfg *c, int variant) {
    memset(c, 0, sizeof(*c));
    c->variant = variant;
    c->uniform = 0;
    c->nUE = 100000;
    c->nPreamble = 54;
    c->backoff = 20;
    c->nGrantUL = variant == PRACH_VARIANT_BETA_C ? 54 : 12;
    c->maxRarWindow = 6;
    c->maxMsg2TxCount = 9;
    c->accessTime = 5;
    c->rng_mode = PRACH_RNG_GLIBC;
    c->seed = 0;
    c->stream_offset = 0;
    c->cellRadius = 400.0f;
    c->hBS = 10.0f;
    c->hUT = 1.8f;
    if (variant == PRACH_VARIANT_NOMA_C) { /* NOMA.c:41-57 */
        c->nGrantUL = 2;        /* per sector */
        c->maxRarWindow = 5;
        c->maxMsg2TxCount = 10; /* maxMsg1ReTx */
        c->cellRadius = 500.0f;
        c->rng_mode = PRACH_RNG_PHILOX;
    }
}

int prach_cfg_validate(const prach_cfg *c) {
    if (!c) return PRACH_ERR_ARG;
    if (c->variant != PRACH_VARIANT_BETA_C && c->variant != PRACH_VARIANT_WITHNOMA_C && c->variant != PRACH_VARIANT_NOMA_C)
        return PRACH_ERR_ARG;
    if (c->nUE < 1 || c->nPreamble < 1 || c->backoff < 1 || c->nGrantUL < 1 || c->accessTime < 1) return PRACH_ERR_ARG;
    if (c->maxRarWindow < 1 || c->maxMsg2TxCount < 0 || c->max_steps < 0) return PRACH_ERR_ARG;
    if (c->rng_mode != PRACH_RNG_GLIBC && c->rng_mode != PRACH_RNG_PHILOX) return PRACH_ERR_ARG;
    if (c->nPreamble > 254 || c->maxRarWindow > 255 || c->maxMsg2TxCount > 255) return PRACH_ERR_UNSUPPORTED;
    if (c->nUE > (1 << 24)) return PRACH_ERR_UNSUPPORTED;
    if (c->flags & ~(PRACH_FLAG_SECTOR_GRANTS | PRACH_FLAG_NOMA_NONSECTOR)) return PRACH_ERR_ARG;
    if ((c->flags & PRACH_FLAG_SECTOR_GRANTS) && c->variant != PRACH_VARIANT_WITHNOMA_C) return PRACH_ERR_ARG; /* sectors exist in that program only */
    if ((c->flags & PRACH_FLAG_NOMA_NONSECTOR) && c->variant != PRACH_VARIANT_NOMA_C) return PRACH_ERR_ARG;
    /* NOMA.c:167-172 redraws the UE's distance until it exceeds 35 m: with a cell radius of 35 m or less the reference itself never returns */
    if (c->variant == PRACH_VARIANT_NOMA_C && !(c->cellRadius > 35.0f && c->cellRadius < 1e9f)) return PRACH_ERR_ARG;
    return PRACH_OK;
}

int prach_max_time(const prach_cfg *c) { return c->uniform ? 60000 : 10000; } /* Beta.c:92,103 */

/* What a trial costs inside a batched launch, in kernel microseconds: the unit the multi-GPU dealing balances (dist.py shard_trials, prach_sim --gpus).
   Measured on an MI355X, 1024 trials of one size per call (scripts/gpu_cost_table.py -> profiles/r04_cost_table.json): the Beta.c program as committed (54 UL
   grants: every UE is served, cost grows with the contention of the big points) and RandomAccessWithNOMA's defaults (12 grants: overloaded from 20 000 UEs
   on, linear in nUE); linear between the sweep's points, proportional beyond them, scaled by the subframes a shortened trial runs.  Uniform arrivals
   (60 000 subframes, a handful of live UEs each) and NOMA.c are costed by size alone: their sweeps deal evenly whatever the constant. */
double prach_trial_cost(const prach_cfg *c) {
    static const double beta_us[10] = {55.67, 81.6, 93.88, 105.34, 119.79, 156.88, 221.75, 293.07, 373.64, 455.66};
    static const double over_us[10] = {57.24, 142.01, 219.44, 298.18, 376.92, 457.74, 538.67, 617.48, 693.07, 769.03};
    const double n = (double)c->nUE;
    const int maxt = prach_max_time(c);
    const double frac = (c->max_steps > 0 && c->max_steps < maxt) ? (double)c->max_steps / (double)maxt : 1.0;
    if (c->variant == PRACH_VARIANT_NOMA_C) return 2.0e-3 * n * frac;
    if (c->uniform) return 1.2e-3 * n * frac;
    /* overloaded: more UEs than the UL grants of the whole trial can serve (nGrantUL - 1 per 5 ms window, Beta.c:112,336) */
    const double capacity = (double)(c->nGrantUL > 1 ? c->nGrantUL - 1 : 0) * (double)maxt / 5.0;
    const double *tab = (c->variant == PRACH_VARIANT_WITHNOMA_C || n > capacity) ? over_us : beta_us;
    double x = n / 10000.0 - 1.0; /* position in the table: 0 at nUE = 10 000 */
    if (x <= 0.0) return tab[0] * n / 10000.0 * frac;
    if (x >= 9.0) return tab[9] * n / 100000.0 * frac;
    const int k = (int)x;
    return (tab[k] + (tab[k + 1] - tab[k]) * (x - (double)k)) * frac;
}

const char *prach_strerror(int s) {
    switch (s) {
    case PRACH_OK: return "ok";
    case PRACH_ERR_ARG: return "invalid argument";
    case PRACH_ERR_UNSUPPORTED: return "parameter outside the supported range (nPreamble<=254, maxRarWindow<=255, maxMsg2TxCount<=255, nUE<=2^24; NOMA_C: nPreamble<=64, Beta arrivals)";
    case PRACH_ERR_DEVICE: return "HIP device/runtime error (an MI355X/gfx950 device is required; there is no CPU fallback)";
    case PRACH_ERR_STREAM: return "glibc draw stream exhausted";
    case PRACH_ERR_INTERNAL: return "device-side consistency check failed";
    case PRACH_ERR_IO: return "I/O error";
    case PRACH_ERR_TIMEOUT: return "a workgroup of a cluster waited too long for a peer (cluster not co-resident)";
    default: return "unknown status";
    }
}

/* Arrival process.  Beta: every accessTime ms, activeCheck += ceil(nUE * pdf(t/maxTime) / (maxTime/accessTime))
 * with the reference's mixed float/double evaluation (Beta.c:127-128, beta_dist Beta.c:516-519:
 * the normaliser is the literal 0.0165, `1 - x` is a float subtraction, pow() runs in double, the
 * product is rounded to float on return).  Uniform: += ceil(n*accessTime/60000), min 1 (Beta.c:95-100).
 * The process uses no random numbers, so it is a table. */
static float beta34_density(float x) {
    const float a = 3, b = 4;
    float v = (1 / 0.0165) * (pow(x, (a - 1))) * (pow((1 - x), (b - 1)));
    return v;
}

int prach_arrival_schedule(const prach_cfg *c, int32_t *out, int cap, int32_t *nAccessUEo) {
    const int nUE = c->nUE, aT = c->accessTime, maxTime = prach_max_time(c);
    int nAccessUE = 0;
    if (c->uniform) {
        nAccessUE = ceil((float)nUE * (float)aT * 1.0 / (float)maxTime);
        if (nAccessUE <= 0) nAccessUE = 1;
    }
    if (nAccessUEo) *nAccessUEo = nAccessUE;
    int activeCheck = 0, s = 0;
    for (int time = 0; time < maxTime; time += aT, s++) {
        if (activeCheck < nUE) {
            if (c->uniform) {
                activeCheck += nAccessUE;
            } else {
                float pdf = beta34_density((float)time / (float)maxTime);
                activeCheck += (int)ceil((float)nUE * pdf / ((float)maxTime / (float)aT));
            }
            if (activeCheck >= nUE) activeCheck = nUE;
        }
        if (s < cap) out[s] = activeCheck;
    }
    return s;
}

/* glibc srand()/rand() (stdlib/random_r.c, TYPE_3: degree 31, separation 3, 310 warm-up draws).
 * The reference links libc's rand(); reproducing its exact stream is what makes per-trial counts
 * bit-exact "under identical seeds".  Checked against libc itself in tests/test_host_logic.py. */
void prach_glibc_stream(uint32_t seed, uint64_t first, uint64_t n, int32_t *out) {
    uint32_t r[31];
    int32_t word = (int32_t)(seed == 0 ? 1u : seed);
    r[0] = (uint32_t)word;
    for (int i = 1; i < 31; i++) {
        int32_t hi = word / 127773, lo = word % 127773;
        word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r[i] = (uint32_t)word;
    }
    int f = 3, b = 0;
    const uint64_t skip = 310 + first;
    for (uint64_t k = 0; k < skip + n; k++) {
        r[f] += r[b];
        if (k >= skip) out[k - skip] = (int32_t)(r[f] >> 1);
        if (++f == 31) f = 0;
        if (++b == 31) b = 0;
    }
}

/* ---- NOMA.c activation table ---------------------------------------------------------------- */
static uint32_t philox31(uint64_t seed, uint32_t nUE, uint32_t variant, uint32_t ue, uint32_t k) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    uint32_t c0 = ue, c1 = k, c2 = nUE, c3 = variant, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0 >> 1;
}

int prach_noma_activation_table(const prach_cfg *c, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                uint32_t *ndraws) {
    if (!c) return PRACH_ERR_ARG;
    return prach_noma_activation_range(c, 0, c->nUE, preamble0, sector, gain, lgain, ndraws);
}

/* UEs [lo, hi) of the table (outputs indexed from lo): every UE's draws are its own Philox counter, so ranges are
 * independent and the engine deals them to all host cores. */
int prach_noma_activation_range(const prach_cfg *c, int lo, int hi, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                uint32_t *ndraws) {
    if (!c || !preamble0 || !sector || !gain || !lgain || !ndraws || lo < 0 || hi > c->nUE || lo > hi) return PRACH_ERR_ARG;
    preamble0 -= lo; sector -= lo; gain -= lo; lgain -= lo; ndraws -= lo;
    const float pi = 3.14; /* NOMA.c:55 */
    const float cellRadius = c->cellRadius;
    for (int i = lo; i < hi; i++) {
        uint32_t k = 0;
#define DRAW() ((int)philox31(c->seed, (uint32_t)c->nUE, PRACH_VARIANT_NOMA_C, (uint32_t)i, k++))
        preamble0[i] = DRAW() % c->nPreamble; /* NOMA.c:133 */
        float angle = (float)DRAW() / (float)(2147483647) * 2 * pi; /* NOMA.c:142 */
        int sec;
        if (angle >= 0 && angle < ((1. / 3.) * pi)) sec = 0; /* NOMA.c:146-163 */
        else if (angle >= ((1. / 3.) * pi) && angle < ((2. / 3.) * pi)) sec = 1;
        else if (angle >= ((2. / 3.) * pi) && angle < 3.14) sec = 2;
        else if (angle >= pi && angle < ((4. / 3.) * pi)) sec = 3;
        else if (angle >= ((4. / 3.) * pi) && angle < ((5. / 3.) * pi)) sec = 4;
        else sec = 5;
        sector[i] = sec;
        float r;
        while (1) { /* NOMA.c:167-172 */
            r = cellRadius * sqrt((float)DRAW() / (float)2147483647);
            if (r > 35.0) break;
        }
        float x = r * cos(angle), y = r * sin(angle), pathloss; /* NOMA.c:176-178 */
        double env = sqrt(x * x + y * y);
        double ch_g = 0, rayleigh;
        while (ch_g < 1e-7) { /* NOMA.c:185-189 */
            pathloss = sqrt(1 + pow(env, 2));
            rayleigh = sqrt(-2 * log((double)DRAW() / (double)2147483647));
            ch_g = pow(rayleigh / pathloss, 2);
        }
#undef DRAW
        gain[i] = ch_g;
        lgain[i] = log(ch_g);
        ndraws[i] = k;
    }
    return PRACH_OK;
}

/* activeUE (NOMA.c:131-192) for ONE UE in the reference's own rand() stream: the draws are stream[*pos], stream[*pos + 1], ... in the
 * order the reference consumes them (preamble, angle, the radius rejection loop, the Rayleigh-gain rejection loop); *pos advances by the
 * number consumed.  Used by the glibc-mode NOMA path (prach_noma_glibc.hip), where the host activates the arrivals of an access slot between
 * two device steps, with the same libm the reference links.  PRACH_ERR_STREAM: the window is exhausted (the engine retries with a larger one). */
int prach_noma_activation_stream(const prach_cfg *c, const int32_t *stream, uint64_t *pos, uint64_t avail, int32_t *preamble0, int32_t *sector,
                                 double *gain, double *lgain) {
    if (!c || !stream || !pos || !preamble0 || !sector || !gain || !lgain) return PRACH_ERR_ARG;
    const float pi = 3.14; /* NOMA.c:55 */
    const float cellRadius = c->cellRadius;
    uint64_t k = *pos;
#define DRAW() (k < avail ? (int)stream[k++] : (k++, -1))
    *preamble0 = DRAW() % c->nPreamble; /* NOMA.c:133 */
    float angle = (float)DRAW() / (float)(2147483647) * 2 * pi; /* NOMA.c:142 */
    int sec;
    if (angle >= 0 && angle < ((1. / 3.) * pi)) sec = 0; /* NOMA.c:146-163 */
    else if (angle >= ((1. / 3.) * pi) && angle < ((2. / 3.) * pi)) sec = 1;
    else if (angle >= ((2. / 3.) * pi) && angle < 3.14) sec = 2;
    else if (angle >= pi && angle < ((4. / 3.) * pi)) sec = 3;
    else if (angle >= ((4. / 3.) * pi) && angle < ((5. / 3.) * pi)) sec = 4;
    else sec = 5;
    *sector = sec;
    float r;
    while (1) { /* NOMA.c:167-172 */
        if (k >= avail) return PRACH_ERR_STREAM;
        r = cellRadius * sqrt((float)DRAW() / (float)2147483647);
        if (r > 35.0) break;
    }
    float x = r * cos(angle), y = r * sin(angle), pathloss; /* NOMA.c:176-178 */
    double env = sqrt(x * x + y * y);
    double ch_g = 0, rayleigh;
    while (ch_g < 1e-7) { /* NOMA.c:185-189 */
        if (k >= avail) return PRACH_ERR_STREAM;
        pathloss = sqrt(1 + pow(env, 2));
        rayleigh = sqrt(-2 * log((double)DRAW() / (double)2147483647));
        ch_g = pow(rayleigh / pathloss, 2);
    }
#undef DRAW
    if (k > avail) return PRACH_ERR_STREAM;
    *gain = ch_g;
    *lgain = log(ch_g);
    *pos = k;
    return PRACH_OK;
}

size_t prach_format_noma_line(const prach_cfg *c, const prach_result *r, char *buf, size_t cap) {
    char tmp[256];
    int n = snprintf(tmp, sizeof tmp, "%d %d %lf %lf %lf\n", c->nUE, r->nSuccessUE, ((float)r->nSuccessUE / (float)c->nUE) * 100.0,
                     ((float)r->preambleTxCount / (float)r->nSuccessUE), ((float)(int)r->sumTimer / (float)r->nSuccessUE));
    if (buf && (size_t)n < cap) memcpy(buf, tmp, (size_t)n + 1);
    return (size_t)n;
}

/* ---- glibc rand() stream: jump-ahead (for the device-side generator) ------------------------------
 * Linear form of the TYPE_3 generator: r[0..30] from the seed, r[31..33] = r[0..2],
 * r[i] = r[i-31] + r[i-3] (mod 2^32) for i >= 34, and the k-th rand() = r[344+k] >> 1.  A window
 * W_n = (r[n-30] .. r[n]) advances by the 31x31 companion matrix A over Z/2^32, so W_{n+D} = A^D W_n:
 * powers A^(2^j) are cached, a jump costs <= 40 mat-vecs.  prach_internal_glibc_seeds returns, for each
 * chunk c of `chunk` outputs starting at output `first`, the window that precedes its first value. */
typedef struct { uint32_t m[31][31]; } lfg_mat;
static lfg_mat lfg_pow2[48];
static pthread_once_t lfg_pow2_once = PTHREAD_ONCE_INIT; /* engines of several host threads may need it at once */

static void lfg_matmul(const lfg_mat *a, const lfg_mat *b, lfg_mat *out) {
    for (int i = 0; i < 31; i++)
        for (int j = 0; j < 31; j++) {
            uint32_t acc = 0;
            for (int k = 0; k < 31; k++) acc += a->m[i][k] * b->m[k][j];
            out->m[i][j] = acc;
        }
}
static void lfg_matvec(const lfg_mat *a, const uint32_t *w, uint32_t *out) {
    for (int i = 0; i < 31; i++) {
        uint32_t acc = 0;
        for (int k = 0; k < 31; k++) acc += a->m[i][k] * w[k];
        out[i] = acc;
    }
}
static void lfg_build_pows(void) {
    memset(&lfg_pow2[0], 0, sizeof(lfg_mat));
    for (int j = 0; j < 30; j++) lfg_pow2[0].m[j][j + 1] = 1; /* w'[j] = w[j+1] */
    lfg_pow2[0].m[30][0] = 1; lfg_pow2[0].m[30][28] = 1;      /* w'[30] = r[n+1] = r[n-30] + r[n-2] = w[0] + w[28] */
    for (int j = 1; j < 48; j++) lfg_matmul(&lfg_pow2[j - 1], &lfg_pow2[j - 1], &lfg_pow2[j]);
}
static void lfg_init_pows(void) { pthread_once(&lfg_pow2_once, lfg_build_pows); }
static void lfg_jump(uint32_t *w, uint64_t d) {
    uint32_t t[31];
    for (int j = 0; d; j++, d >>= 1)
        if (d & 1) { lfg_matvec(&lfg_pow2[j], w, t); memcpy(w, t, sizeof t); }
}

void prach_internal_glibc_seeds(uint32_t seed, uint64_t first, uint64_t nchunks, uint64_t chunk, uint32_t *out /* [nchunks][31] */) {
    lfg_init_pows();
    uint32_t r[34];
    int32_t word = (int32_t)(seed == 0 ? 1u : seed);
    r[0] = (uint32_t)word;
    for (int i = 1; i < 31; i++) {
        int32_t hi = word / 127773, lo = word % 127773;
        word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r[i] = (uint32_t)word;
    }
    r[31] = r[0]; r[32] = r[1]; r[33] = r[2];
    uint32_t w[31];
    for (int j = 0; j < 31; j++) w[j] = r[3 + j];         /* W_33 */
    lfg_jump(w, 310ull + first);                           /* W_{343+first}: the next value is r[344+first] */
    lfg_mat step;
    {   /* A^chunk */
        lfg_mat acc, tmp;
        memset(&acc, 0, sizeof acc);
        for (int i = 0; i < 31; i++) acc.m[i][i] = 1;
        uint64_t d = chunk;
        for (int j = 0; d; j++, d >>= 1)
            if (d & 1) { lfg_matmul(&lfg_pow2[j], &acc, &tmp); acc = tmp; }
        step = acc;
    }
    for (uint64_t c = 0; c < nchunks; c++) {
        memcpy(out + c * 31, w, sizeof w);
        uint32_t t[31];
        lfg_matvec(&step, w, t);
        memcpy(w, t, sizeof t);
    }
}

/* ---- text surfaces ---------------------------------------------------------------------------- */

/* The per-UE log is 24 MB of text per 100k-UE trial (Beta.c:501-508): once the trial itself takes 85 ms the formatter is
 * what the caller waits for, so the line is assembled by hand (fixed labels + decimal integers) instead of snprintf. */
static char *put_int(char *p, int32_t v) {
    uint32_t u = (uint32_t)v;
    if (v < 0) { *p++ = '-'; u = 0u - u; }
    char tmp[10];
    int n = 0;
    do { tmp[n++] = (char)('0' + u % 10u); u /= 10u; } while (u);
    while (n) *p++ = tmp[--n];
    return p;
}
#define PUT_LIT(s) do { memcpy(p, s, sizeof(s) - 1); p += sizeof(s) - 1; } while (0)
#define PRACH_LOG_LINE_MAX 384 /* 213 bytes of labels and newline + 15 integers of at most 11 characters = 378 */

static size_t format_log_line(const prach_ue_log *u, char *line) {
    char *p = line;
    PUT_LIT("Idx: "); p = put_int(p, u->idx);
    PUT_LIT(" | Timer: "); p = put_int(p, u->timer);
    PUT_LIT(" | Active: "); p = put_int(p, u->active);
    PUT_LIT(" | txTime: "); p = put_int(p, u->txTime);
    PUT_LIT(" | FirstTxTime: "); p = put_int(p, u->firstTxTime);
    PUT_LIT(" | SecondTxTime: "); p = put_int(p, u->secondTxTime);
    PUT_LIT(" | NowBackoff: "); p = put_int(p, u->nowBackoff);
    PUT_LIT(" | Preamble: "); p = put_int(p, u->preamble);
    PUT_LIT(" | Preamble change: "); p = put_int(p, u->preambleChange);
    PUT_LIT(" | RAR window: "); p = put_int(p, u->rarWindow);
    PUT_LIT(" | Max RAR: "); p = put_int(p, u->maxRarCounter);
    PUT_LIT(" | Preamble reTx: "); p = put_int(p, u->preambleTxCounter);
    PUT_LIT(" | MSG 2 Flag: "); p = put_int(p, u->msg2Flag);
    PUT_LIT(" | ConnectRequest: "); p = put_int(p, u->connectionRequest);
    PUT_LIT(" | MSG 4 Flag: "); p = put_int(p, u->msg4Flag);
    *p++ = '\n';
    return (size_t)(p - line);
}

size_t prach_format_logs(const prach_ue_log *ue, int nUE, char *buf, size_t cap) {
    size_t off = 0;
    char line[PRACH_LOG_LINE_MAX];
    for (int i = 0; i < nUE; i++) {
        if (buf && off + PRACH_LOG_LINE_MAX <= cap) { /* room for any line: format in place */
            off += format_log_line(ue + i, buf + off);
            continue;
        }
        const size_t n = format_log_line(ue + i, line);
        if (buf && off + n <= cap) memcpy(buf + off, line, n);
        off += n;
    }
    return off;
}

typedef struct { float ratioSuccess, nCollisionPreambles, averagePreambleTx, averageDelay; } derived_t;

/* the float arithmetic of saveSimulationLog (Beta.c:434-438) */
static derived_t derive(const prach_cfg *c, const prach_result *r) {
    derived_t d;
    d.ratioSuccess = (float)r->nSuccessUE / (float)c->nUE * 100.0;
    d.nCollisionPreambles = (float)r->collisionPreambles / ((float)c->nUE * (float)c->nPreamble);
    d.averagePreambleTx = (float)r->preambleTxCount / (float)r->nSuccessUE;
    d.averageDelay = r->totalDelay / (float)r->nSuccessUE;
    return d;
}

size_t prach_format_results(const prach_cfg *c, const prach_result *r, double latency_s, char *buf, size_t cap) {
    derived_t d = derive(c, r);
    char tmp[1024];
    int n;
    if (c->variant == PRACH_VARIANT_WITHNOMA_C)
        n = snprintf(tmp, sizeof tmp,
                     "%d\n%.2lf\n%d\n%.2lf\n%.2lf\nNumber of total preamble tx: %d\nFinally Falied: %d\nFinally Success: %lf\n",
                     c->nUE, d.ratioSuccess, r->nSuccessUE, d.averagePreambleTx, d.averageDelay, r->preambleTxCount,
                     r->continueFaliedUEs,
                     (float)r->finalSuccessUEs / (float)(r->continueFaliedUEs + r->finalSuccessUEs));
    else
        n = snprintf(tmp, sizeof tmp, "%d\n%.2lf\n%d\n%.2lf\n%.2lf\n%lf", c->nUE, d.ratioSuccess, r->nSuccessUE,
                     d.averagePreambleTx, d.averageDelay, latency_s);
    if (buf && (size_t)n < cap) memcpy(buf, tmp, (size_t)n + 1);
    return (size_t)n;
}

size_t prach_format_stdout(const prach_cfg *c, const prach_result *r, double latency_s, char *buf, size_t cap) {
    derived_t d = derive(c, r);
    char tmp[2048];
    int n = snprintf(tmp, sizeof tmp, "-------- %05d Result ---------\n", r->activeCheck);
    if (c->uniform) n += snprintf(tmp + n, sizeof tmp - n, "Number of RA try UEs per Subframe: %d\n", r->nAccessUE);
    if (c->variant == PRACH_VARIANT_WITHNOMA_C) n += snprintf(tmp + n, sizeof tmp - n, "Fail Counts: %d\n", r->failCounts);
    else n += snprintf(tmp + n, sizeof tmp - n, "Latency: %lf\n", latency_s);
    n += snprintf(tmp + n, sizeof tmp - n,
                  "Number of UEs: %d\nTotal simulation time: %dms\nSuccess ratio: %.2lf\nNumber of succeed UEs: %d\n", c->nUE,
                  r->time_exit, d.ratioSuccess, r->nSuccessUE);
    if (c->variant == PRACH_VARIANT_WITHNOMA_C)
        n += snprintf(tmp + n, sizeof tmp - n, "Number of falied UEs: %d\n", r->continueFaliedUEs);
    n += snprintf(tmp + n, sizeof tmp - n,
                  "Number of collision preambles: %.6lf\nAverage preamble tx count: %.2lf\nAverage delay: %.2lf\n",
                  d.nCollisionPreambles, d.averagePreambleTx, d.averageDelay);
    if (buf && (size_t)n < cap) memcpy(buf, tmp, (size_t)n + 1);
    return (size_t)n;
}

/* Output file names: Beta.c:452-456,490-494 and WithNOMA:754-758,801-805 (note Beta.c's Uniform log
 * name has no seed in it). */
int prach_result_file_name(const prach_cfg *c, int is_log, char *buf, size_t cap) {
    const int seed = (int)c->seed;
    int n;
    if (c->variant == PRACH_VARIANT_WITHNOMA_C) {
        const char *dir = c->uniform ? "NomaUniformResults" : "NomaBetaResults";
        n = is_log ? snprintf(buf, cap, "%s/%d_%d_UE%05d_Logs.txt", dir, seed, c->nPreamble, c->nUE)
                   : snprintf(buf, cap, "%s/%d_%d_%d_Results.txt", dir, seed, c->nPreamble, c->nUE);
    } else {
        const char *dir = c->uniform ? "BasicUniformSimulationResults" : "BasicBetaSimulationResults";
        if (!is_log) n = snprintf(buf, cap, "%s/%d_%d_%d_Results.txt", dir, seed, c->nPreamble, c->nUE);
        else if (c->uniform) n = snprintf(buf, cap, "%s/%d_Exclude_msg2_failures_UE%05d_Logs.txt", dir, c->nPreamble, c->nUE);
        else n = snprintf(buf, cap, "%s/%d_%d_UE%05d_Logs.txt", dir, seed, c->nPreamble, c->nUE);
    }
    return (n > 0 && (size_t)n < cap) ? PRACH_OK : PRACH_ERR_ARG;
}

static int write_all(const char *path, const char *data, size_t n) {
    FILE *fp = fopen(path, "w+");
    if (!fp) return PRACH_ERR_IO;
    size_t w = fwrite(data, 1, n, fp);
    if (fclose(fp) != 0 || w != n) return PRACH_ERR_IO;
    return PRACH_OK;
}

int prach_write_trial_files(const prach_cfg *c, const prach_result *r, const prach_ue_log *ue, double latency_s,
                            const char *root_dir) {
    char rel[512], path[1024], dirp[1024];
    const char *root = (root_dir && *root_dir) ? root_dir : ".";
    int rc = prach_result_file_name(c, 0, rel, sizeof rel);
    if (rc) return rc;
    /* the reference mkdir()s its output directories (WithNOMA:67-68); Beta.c expects them to exist */
    snprintf(dirp, sizeof dirp, "%s/%.*s", root, (int)(strchr(rel, '/') - rel), rel);
    if (mkdir(dirp, 0755) != 0 && errno != EEXIST) return PRACH_ERR_IO;
    char text[1024];
    size_t n = prach_format_results(c, r, latency_s, text, sizeof text);
    snprintf(path, sizeof path, "%s/%s", root, rel);
    if ((rc = write_all(path, text, n)) != 0) return rc;
    if (ue) {
        const size_t cap = (size_t)c->nUE * PRACH_LOG_LINE_MAX + 1;
        char *buf = (char *)malloc(cap);
        if (!buf) return PRACH_ERR_IO;
        const size_t need = prach_format_logs(ue, c->nUE, buf, cap);
        prach_result_file_name(c, 1, rel, sizeof rel);
        snprintf(path, sizeof path, "%s/%s", root, rel);
        rc = write_all(path, buf, need);
        free(buf);
    }
    return rc;
}

/* ---- results.csv (AveragePerformance.py) ------------------------------------------------------ */

int prach_results_csv_accumulate(double acc[6], const char *txt) {
    if (!acc || !txt) return PRACH_ERR_ARG;
    const char *p = txt;
    for (int i = 0; i < 6; i++) { /* data.append(float(line.strip())) for the six lines (AveragePerformance.py:14-19) */
        char *end;
        double v = strtod(p, &end);
        if (end == p) return PRACH_ERR_ARG;
        acc[i] += v;
        p = end;
        while (*p == '\n' || *p == '\r' || *p == ' ') p++;
    }
    return PRACH_OK;
}

/* Python's repr(float): shortest digit string that round-trips, fixed notation for 1e-4 <= |x| < 1e16 */
static int py_float_repr(double x, char *out, size_t cap) {
    if (x == 0) return snprintf(out, cap, signbit(x) ? "-0.0" : "0.0");
    if (!isfinite(x)) return snprintf(out, cap, isnan(x) ? "nan" : (x > 0 ? "inf" : "-inf"));
    char e[40];
    int prec;
    for (prec = 1; prec <= 17; prec++) {
        snprintf(e, sizeof e, "%.*e", prec - 1, x);
        if (strtod(e, NULL) == x) break;
    }
    /* e = [-]d.ddddde[+-]XX */
    const char *m = e;
    int neg = 0;
    if (*m == '-') { neg = 1; m++; }
    char digits[24];
    int nd = 0;
    for (; *m && *m != 'e'; m++)
        if (*m >= '0' && *m <= '9') digits[nd++] = *m;
    while (nd > 1 && digits[nd - 1] == '0') nd--; /* shortest */
    int ex = atoi(m + 1);
    char body[64];
    int n = 0;
    if (ex < -4 || ex >= 16) {
        body[n++] = digits[0];
        if (nd > 1) { body[n++] = '.'; for (int i = 1; i < nd; i++) body[n++] = digits[i]; }
        n += snprintf(body + n, sizeof body - n, "e%c%02d", ex < 0 ? '-' : '+', ex < 0 ? -ex : ex);
    } else if (ex >= 0) {
        for (int i = 0; i <= ex; i++) body[n++] = i < nd ? digits[i] : '0';
        body[n++] = '.';
        if (nd > ex + 1) for (int i = ex + 1; i < nd; i++) body[n++] = digits[i];
        else body[n++] = '0';
    } else {
        body[n++] = '0'; body[n++] = '.';
        for (int i = 0; i < -ex - 1; i++) body[n++] = '0';
        for (int i = 0; i < nd; i++) body[n++] = digits[i];
    }
    body[n] = 0;
    return snprintf(out, cap, "%s%s", neg ? "-" : "", body);
}

size_t prach_results_csv_row(const double acc[6], int nseeds, char *buf, size_t cap) {
    char tmp[512];
    int n = 0;
    for (int i = 0; i < 6; i++) {
        double v = acc[i] / (double)nseeds;       /* lists/len(seedNumber) */
        v = rint(v * 1000.0) / 1000.0;             /* np.around(., 3): multiply, rint (half to even), divide */
        char f[80];
        py_float_repr(v, f, sizeof f);
        n += snprintf(tmp + n, sizeof tmp - n, "%s%s", i ? "," : "", f);
    }
    n += snprintf(tmp + n, sizeof tmp - n, "\r\n"); /* csv.writer default line terminator */
    if (buf && (size_t)n < cap) memcpy(buf, tmp, (size_t)n + 1);
    return (size_t)n;
}

/* ---- the CSV text of a reduction: one line at a time into buf[cap]; the size is counted also where nothing (more) fits ---- */

__attribute__((format(printf, 4, 5))) static int csv_emit(char *buf, size_t cap, size_t *off, const char *fmt, ...) {
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    if (n < 0 || (size_t)n >= sizeof line) return 0;
    if (buf && *off + (size_t)n < cap) memcpy(buf + *off, line, (size_t)n);
    *off += (size_t)n;
    return 1;
}
#define CSV_EMIT(...) do { if (!csv_emit(buf, cap, &off, __VA_ARGS__)) return 0; } while (0)
static size_t csv_end(char *buf, size_t cap, size_t off) {
    if (buf && off < cap) buf[off] = 0;
    else if (buf && cap) buf[0] = 0; /* (did not fit: nothing partial is left behind as a string) */
    return off;
}

/* a kind's shape function (prach_grouped.h) is the judge of its spec */
static int spec_ok(int (*shape)(const void *, size_t *), const void *spec) {
    size_t words[PRACH_G_MAX_ARRAYS];
    return shape(spec, words) != 0;
}

/* ---- distributions of the successful UEs (prach_run_trials_dist) -------------------------------- */

static int dist_shape(const void *spec, size_t words[]) {
    const prach_dist_spec *s = (const prach_dist_spec *)spec;
    if (!s || s->delay_bins < 1 || s->delay_bins > PRACH_DIST_MAX_DELAY_BINS || s->delay_bin_ms < 1) return 0;
    words[0] = (size_t)s->delay_bins; words[1] = PRACH_DIST_PTC_BINS;
    return 2;
}

/* one successful UE (timer >= 0): what prach::dist_kernel does per lane */
void prach_internal_dist_add_ue(const prach_dist_spec *s, prach_dist *d, uint64_t *delay_hist, uint64_t *ptc_hist, int32_t timer, int32_t ptc) {
    const int64_t b = (int64_t)timer / s->delay_bin_ms;
    if (b < s->delay_bins) delay_hist[b]++;
    else d->delay_overflow++;
    ptc_hist[(uint32_t)ptc < PRACH_DIST_PTC_BINS - 1 ? ptc : PRACH_DIST_PTC_BINS - 1]++;
    d->success++;
    d->delay_sum += (uint64_t)timer;
    d->ptc_sum += (uint64_t)(uint32_t)ptc;
    if (timer > d->delay_max) d->delay_max = timer;
}

int prach_dist_accumulate_logs(const prach_dist_spec *s, const prach_ue_log *ue, int nUE, prach_dist *d, uint64_t *delay_hist, uint64_t *ptc_hist) {
    if (!spec_ok(dist_shape, s) || !d || !delay_hist || !ptc_hist || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    for (int i = 0; i < nUE; i++)
        if (ue[i].msg4Flag == 1 && ue[i].timer < 0) return PRACH_ERR_ARG;
    if (d->trials == 0 && d->success == 0) d->delay_max = -1; /* (a zero-filled group is an empty one) */
    for (int i = 0; i < nUE; i++)
        if (ue[i].msg4Flag == 1) prach_internal_dist_add_ue(s, d, delay_hist, ptc_hist, ue[i].timer, ue[i].preambleTxCounter);
    d->trials++;
    d->ues += (uint64_t)nUE;
    return PRACH_OK;
}

int64_t prach_dist_delay_quantile(const prach_dist_spec *s, const prach_dist *d, const uint64_t *delay_hist, double q) {
    if (!spec_ok(dist_shape, s) || !d || !delay_hist || d->success == 0 || !(q >= 0.0) || q > 1.0) return -1;
    uint64_t rank = (uint64_t)ceil(q * (double)d->success);
    if (rank < 1) rank = 1;
    if (rank > d->success) rank = d->success;
    uint64_t cum = 0;
    for (int b = 0; b < s->delay_bins; b++) {
        cum += delay_hist[b];
        if (cum >= rank) return (int64_t)b * s->delay_bin_ms;
    }
    return -1; /* in the overflow */
}

static size_t dist_csv(const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap) {
    const prach_dist_spec *s = (const prach_dist_spec *)spec;
    const prach_dist *d = (const prach_dist *)group;
    const uint64_t *const delay_hist = arrays[0], *const ptc_hist = arrays[1];
    size_t off = 0;
    const double tot = d->success ? (double)d->success : 1.0;
    uint64_t cum = 0;
    for (int b = 0; b < s->delay_bins; b++) {
        if (!delay_hist[b]) continue;
        cum += delay_hist[b];
        CSV_EMIT("%.200s,delay,%lld,%llu,%.6f\n", label, (long long)b * s->delay_bin_ms, (unsigned long long)delay_hist[b], (double)cum / tot);
    }
    if (d->delay_overflow) CSV_EMIT("%.200s,delay,overflow,%llu,1.000000\n", label, (unsigned long long)d->delay_overflow);
    cum = 0;
    for (int k = 0; k < PRACH_DIST_PTC_BINS; k++) {
        if (!ptc_hist[k]) continue;
        cum += ptc_hist[k];
        CSV_EMIT("%.200s,ptx,%d,%llu,%.6f\n", label, k, (unsigned long long)ptc_hist[k], (double)cum / tot);
    }
    return csv_end(buf, cap, off);
}

/* ---- the four kinds of series by time (timeline, trace, noma_trace, noma_timeline): one shape, one formatter ---- */

/* nseries arrays of sectors * bins words each */
static int series_shape(int bins, int bin_ms, int max_bins, int nseries, int sectors, size_t words[]) {
    if (bins < 1 || bins > max_bins || bin_ms < 1) return 0;
    for (int q = 0; q < nseries; q++) words[q] = (size_t)sectors * (size_t)bins;
    return nseries;
}

/* a kind's lines: its series in order, a line per non-zero bin (per sector and over all sectors where there are 6); behind series `after` an overflow line
   under the name of series `name`, from the counter at byte `at` of the group struct if that is non-zero */
typedef struct series_overflow { int after, name; size_t at; } series_overflow;
typedef struct series_lines {
    const char *const *names;
    int nseries, sectors, noverflow;
    series_overflow overflow[2];
} series_lines;
static size_t series_csv(const series_lines *k, int bins, int bin_ms, const void *group, const uint64_t *const series[], const char *label, char *buf, size_t cap) {
    size_t off = 0;
    for (int q = 0; q < k->nseries; q++) {
        for (int b = 0; b < bins; b++) {
            if (k->sectors == 1) {
                if (series[q][b]) CSV_EMIT("%.200s,%s,%lld,%llu\n", label, k->names[q], (long long)b * bin_ms, (unsigned long long)series[q][b]);
                continue;
            }
            uint64_t all = 0;
            for (int c = 0; c < k->sectors; c++) {
                const uint64_t v = series[q][(size_t)c * (size_t)bins + (size_t)b];
                all += v;
                if (v) CSV_EMIT("%.200s,%s,%d,%lld,%llu\n", label, k->names[q], c, (long long)b * bin_ms, (unsigned long long)v);
            }
            if (all) CSV_EMIT("%.200s,%s,all,%lld,%llu\n", label, k->names[q], (long long)b * bin_ms, (unsigned long long)all);
        }
        for (int o = 0; o < k->noverflow; o++) {
            const uint64_t v = *(const uint64_t *)((const char *)group + k->overflow[o].at);
            if (k->overflow[o].after == q && v) CSV_EMIT(k->sectors == 1 ? "%.200s,%s,overflow,%llu\n" : "%.200s,%s,all,overflow,%llu\n", label, k->names[k->overflow[o].name], (unsigned long long)v);
        }
    }
    return csv_end(buf, cap, off);
}

/* ---- timelines per trial group (prach_run_trials_timeline) -------------------------------------- */

static int timeline_shape(const void *spec, size_t words[]) {
    const prach_timeline_spec *s = (const prach_timeline_spec *)spec;
    return s ? series_shape(s->bins, s->bin_ms, PRACH_TIMELINE_MAX_BINS, 5, 1, words) : 0;
}

/* THE DEFINITION (include/prach.h).  Two passes: the first only judges, so that a refused log leaves nothing behind */
int prach_timeline_accumulate_logs(const prach_timeline_spec *s, const prach_cfg *cfg, const prach_ue_log *ue, int nUE, prach_timeline *t, uint64_t *arrivals,
                                   uint64_t *success, uint64_t *sojourn_sum, uint64_t *timer_sum, uint64_t *done) {
    if (!spec_ok(timeline_shape, s) || !cfg || !t || !arrivals || !success || !sojourn_sum || !timer_sum || !done || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    if (cfg->variant == PRACH_VARIANT_NOMA_C) return PRACH_ERR_UNSUPPORTED;
    if (prach_cfg_validate(cfg) != PRACH_OK || nUE != cfg->nUE) return PRACH_ERR_ARG;
    const int nslots = (prach_max_time(cfg) + cfg->accessTime - 1) / cfg->accessTime;
    int32_t *sched = (int32_t *)malloc(sizeof(int32_t) * (size_t)nslots);
    if (!sched) return PRACH_ERR_INTERNAL;
    prach_arrival_schedule(cfg, sched, nslots, NULL);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && t->trials == 0 && t->success == 0) t->done_max = -1; /* (a zero-filled group is an empty one) */
        int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
        for (int i = 0; i < nUE; i++) {
            while (slot < nslots && sched[slot] <= i) slot++;
            const int64_t a = (int64_t)cfg->accessTime * slot;
            const int ok = ue[i].msg4Flag == 1;
            const int64_t c = (int64_t)ue[i].txTime + 6;
            if (pass == 0) {
                if (ue[i].active != -1 && ok && (ue[i].timer < 0 || c < a)) { free(sched); return PRACH_ERR_ARG; }
                continue;
            }
            if (ue[i].active == -1) continue; /* not arrived */
            const int64_t ab = a / s->bin_ms;
            t->arrived++;
            if (ab < s->bins) arrivals[ab]++;
            else t->arrival_overflow++;
            if (!ok) continue;
            const int64_t db = c / s->bin_ms;
            t->success++;
            t->restarted += c - ue[i].timer != a;
            t->sojourn_sum += (uint64_t)(c - a);
            t->timer_sum += (uint64_t)ue[i].timer;
            if (c > t->done_max) t->done_max = c;
            if (ab < s->bins) { success[ab]++; sojourn_sum[ab] += (uint64_t)(c - a); timer_sum[ab] += (uint64_t)ue[i].timer; }
            if (db < s->bins) done[db]++;
            else t->done_overflow++;
        }
    }
    free(sched);
    t->trials++;
    t->ues += (uint64_t)nUE;
    return PRACH_OK;
}

static size_t timeline_csv(const void *spec, const void *group, const uint64_t *const series[], const char *label, char *buf, size_t cap) {
    static const char *const names[5] = {"arrivals", "success", "sojourn_sum", "timer_sum", "done"};
    static const series_lines lines = {names, 5, 1, 2, {{0, 0, offsetof(prach_timeline, arrival_overflow)}, {4, 4, offsetof(prach_timeline, done_overflow)}}};
    const prach_timeline_spec *s = (const prach_timeline_spec *)spec;
    return series_csv(&lines, s->bins, s->bin_ms, group, series, label, buf, cap);
}

/* ---- per-subframe preamble traces per trial group (prach_run_trials_trace) ----------------------- */

static int trace_shape(const void *spec, size_t words[]) {
    const prach_trace_spec *s = (const prach_trace_spec *)spec;
    return s ? series_shape(s->bins, s->bin_ms, PRACH_TRACE_MAX_BINS, 4, 1, words) : 0;
}

static size_t trace_csv(const void *spec, const void *group, const uint64_t *const series[], const char *label, char *buf, size_t cap) {
    static const char *const names[4] = {"calls", "singles", "txop", "collisions"};
    static const series_lines lines = {names, 4, 1, 1, {{3, 0, offsetof(prach_trace, overflow_calls)}, {0, 0, 0}}};
    const prach_trace_spec *s = (const prach_trace_spec *)spec;
    return series_csv(&lines, s->bins, s->bin_ms, group, series, label, buf, cap);
}

/* ---- NOMA.c's channel trace per trial group (prach_run_trials_noma_trace) -------------------------- */

static int noma_trace_shape(const void *spec, size_t words[]) {
    const prach_noma_trace_spec *s = (const prach_noma_trace_spec *)spec;
    return s ? series_shape(s->bins, s->bin_ms, PRACH_TRACE_MAX_BINS, 6, 6, words) : 0;
}

static size_t noma_trace_csv(const void *spec, const void *group, const uint64_t *const series[], const char *label, char *buf, size_t cap) {
    static const char *const names[6] = {"tx", "used", "singles", "granted", "pairs", "pair_one"};
    static const series_lines lines = {names, 6, 6, 1, {{5, 0, offsetof(prach_noma_trace, overflow_tx)}, {0, 0, 0}}};
    const prach_noma_trace_spec *s = (const prach_noma_trace_spec *)spec;
    return series_csv(&lines, s->bins, s->bin_ms, group, series, label, buf, cap);
}

/* ---- sojourn histograms by arrival row per trial group (prach_run_trials_sojourn) ---------------- */

static int sojourn_shape(const void *spec, size_t words[]) {
    const prach_sojourn_spec *s = (const prach_sojourn_spec *)spec;
    if (!s || s->arrival_bins < 1 || s->arrival_bins > PRACH_SOJOURN_MAX_ARRIVAL_BINS || s->arrival_bin_ms < 1 || s->delay_bins < 1 ||
        s->delay_bins > PRACH_SOJOURN_MAX_DELAY_BINS || s->delay_bin_ms < 1) return 0;
    words[0] = (size_t)s->arrival_bins * (size_t)s->delay_bins; words[1] = words[2] = (size_t)s->arrival_bins;
    return 3;
}

/* THE DEFINITION (include/prach.h).  Two passes, like the timeline's: the first only judges, so that a refused log leaves nothing behind */
int prach_sojourn_accumulate_logs(const prach_sojourn_spec *s, const prach_cfg *cfg, const prach_ue_log *ue, int nUE, prach_sojourn *j, uint64_t *hist,
                                  uint64_t *row_arrived, uint64_t *row_delay_overflow) {
    if (!spec_ok(sojourn_shape, s) || !cfg || !j || !hist || !row_arrived || !row_delay_overflow || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    if (cfg->variant == PRACH_VARIANT_NOMA_C) return PRACH_ERR_UNSUPPORTED;
    if (prach_cfg_validate(cfg) != PRACH_OK || nUE != cfg->nUE) return PRACH_ERR_ARG;
    const int nslots = (prach_max_time(cfg) + cfg->accessTime - 1) / cfg->accessTime;
    int32_t *sched = (int32_t *)malloc(sizeof(int32_t) * (size_t)nslots);
    if (!sched) return PRACH_ERR_INTERNAL;
    prach_arrival_schedule(cfg, sched, nslots, NULL);
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && j->trials == 0 && j->success == 0) j->sojourn_max = -1; /* (a zero-filled group is an empty one) */
        int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
        for (int i = 0; i < nUE; i++) {
            while (slot < nslots && sched[slot] <= i) slot++;
            const int64_t a = (int64_t)cfg->accessTime * slot;
            const int ok = ue[i].msg4Flag == 1;
            const int64_t c = (int64_t)ue[i].txTime + 6;
            if (pass == 0) {
                if (ue[i].active != -1 && ok && (ue[i].timer < 0 || c < a)) { free(sched); return PRACH_ERR_ARG; }
                continue;
            }
            if (ue[i].active == -1) continue; /* not arrived */
            const int64_t r = a / s->arrival_bin_ms;
            j->arrived++;
            if (r < s->arrival_bins) row_arrived[r]++;
            else j->arrival_overflow++;
            if (!ok) continue;
            const int64_t soj = c - a, d = soj / s->delay_bin_ms;
            j->success++;
            j->restarted += c - ue[i].timer != a;
            j->sojourn_sum += (uint64_t)soj;
            if (soj > j->sojourn_max) j->sojourn_max = soj;
            if (d >= s->delay_bins) j->delay_overflow++;
            if (r >= s->arrival_bins) continue;
            if (d < s->delay_bins) hist[(size_t)r * (size_t)s->delay_bins + (size_t)d]++;
            else row_delay_overflow[r]++;
        }
    }
    free(sched);
    j->trials++;
    j->ues += (uint64_t)nUE;
    return PRACH_OK;
}

int64_t prach_sojourn_quantile(const prach_sojourn_spec *s, const uint64_t *hist, const uint64_t *row_delay_overflow, int row, double q) {
    if (!spec_ok(sojourn_shape, s) || !hist || !row_delay_overflow || row < -1 || row >= s->arrival_bins || !(q >= 0.0) || q > 1.0) return -1;
    const int r0 = row < 0 ? 0 : row, r1 = row < 0 ? s->arrival_bins : row + 1;
    uint64_t n = 0;
    for (int r = r0; r < r1; r++) {
        n += row_delay_overflow[r];
        for (int d = 0; d < s->delay_bins; d++) n += hist[(size_t)r * (size_t)s->delay_bins + (size_t)d];
    }
    if (n == 0) return -1;
    uint64_t rank = (uint64_t)ceil(q * (double)n);
    if (rank < 1) rank = 1;
    if (rank > n) rank = n;
    uint64_t cum = 0;
    for (int d = 0; d < s->delay_bins; d++) {
        for (int r = r0; r < r1; r++) cum += hist[(size_t)r * (size_t)s->delay_bins + (size_t)d];
        if (cum >= rank) return (int64_t)d * s->delay_bin_ms;
    }
    return -1; /* in the overflow */
}

static size_t sojourn_csv(const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap) {
    const prach_sojourn_spec *s = (const prach_sojourn_spec *)spec;
    const prach_sojourn *j = (const prach_sojourn *)group;
    const uint64_t *const hist = arrays[0], *const row_arrived = arrays[1], *const row_delay_overflow = arrays[2];
    size_t off = 0;
    for (int r = 0; r < s->arrival_bins; r++) {
        const long long edge = (long long)r * s->arrival_bin_ms;
        const uint64_t *const h = hist + (size_t)r * (size_t)s->delay_bins;
        if (row_arrived[r]) CSV_EMIT("%.200s,%lld,arrived,%llu\n", label, edge, (unsigned long long)row_arrived[r]);
        for (int d = 0; d < s->delay_bins; d++)
            if (h[d]) CSV_EMIT("%.200s,%lld,%lld,%llu\n", label, edge, (long long)d * s->delay_bin_ms, (unsigned long long)h[d]);
        if (row_delay_overflow[r]) CSV_EMIT("%.200s,%lld,overflow,%llu\n", label, edge, (unsigned long long)row_delay_overflow[r]);
    }
    if (j->arrival_overflow) CSV_EMIT("%.200s,arrivals,overflow,%llu\n", label, (unsigned long long)j->arrival_overflow);
    return csv_end(buf, cap, off);
}

/* ---- the two menus of per-UE quantities (include/prach.h) and THE DEFINITIONS over them: census, columns, pick ---- */

/* the menu of PRACH_XTAB_*: the class bit of a UE and its STATE */
static int xtab_class(const prach_ue_log *u) {
    return u->active == -1 ? PRACH_XTAB_IDLE : u->msg4Flag == 1 ? PRACH_XTAB_SERVED : PRACH_XTAB_UNSERVED;
}
static int xtab_state(const prach_ue_log *u) {
    const int cls = xtab_class(u);
    if (cls == PRACH_XTAB_IDLE) return 0;
    if (cls == PRACH_XTAB_SERVED) return 1;
    if (u->active == 1) return u->nowBackoff > 0 ? 2 : 3;
    if (u->active == 2) return u->connectionRequest < 48 ? 4 : 5;
    return 6;
}
/* the value of a field for a UE of class cls that arrived at a; a negative value is UNDEFINED, and so is a field outside the classes it is defined for */
static int64_t xtab_value(int field, const prach_ue_log *u, int cls, int64_t a, int64_t E) {
    const int arrived = cls != PRACH_XTAB_IDLE, served = cls == PRACH_XTAB_SERVED;
    switch (field) {
    case PRACH_XTAB_ONE: return 0;
    case PRACH_XTAB_ARRIVAL: return arrived ? a : -1;
    case PRACH_XTAB_SOJOURN: return served ? (int64_t)u->txTime + 6 - a : -1;
    case PRACH_XTAB_COMPLETION: return served ? (int64_t)u->txTime + 6 : -1;
    case PRACH_XTAB_TIMER: return arrived ? u->timer : -1;
    case PRACH_XTAB_PTC: return arrived ? u->preambleTxCounter : -1;
    case PRACH_XTAB_FAILCOUNT: return arrived ? u->failCount : -1;
    case PRACH_XTAB_AGE: return arrived ? E - a : -1;
    default: return xtab_state(u);
    }
}

/* the menu of PRACH_NOMA_*: the class bit of a UE and its STATE */
static int noma_class(const prach_ue_log *u) {
    if (u->preambleChange == -1) return PRACH_NOMA_IDLE;
    if (u->msg4Flag == 1) return PRACH_NOMA_SERVED;
    return (u->failCount & 0xffff) != 0 ? PRACH_NOMA_DROPPED : PRACH_NOMA_PENDING;
}
static int noma_state(const prach_ue_log *u, int cls, int64_t E) {
    if (cls == PRACH_NOMA_IDLE) return 0;
    if (cls == PRACH_NOMA_SERVED) return 1;
    if (cls == PRACH_NOMA_DROPPED) return 2;
    if (u->active == 1) return u->nowBackoff > 0 ? 3 : (int64_t)u->txTime >= E ? 4 : 5;
    if (u->active == 2) return u->connectionRequest == 0 ? 6 : 7;
    return 8;
}
static int64_t noma_value(int field, const prach_ue_log *u, int cls, int64_t a, int64_t E) {
    const int arrived = cls != PRACH_NOMA_IDLE, served = cls == PRACH_NOMA_SERVED;
    switch (field) {
    case PRACH_NOMA_ONE: return 0;
    case PRACH_NOMA_ARRIVAL: return arrived ? a : -1;
    case PRACH_NOMA_SOJOURN: return served ? (int64_t)u->txTime + 6 - a : -1;
    case PRACH_NOMA_COMPLETION: return served ? (int64_t)u->txTime + 6 : -1;
    case PRACH_NOMA_TIMER: return arrived ? u->timer : -1;
    case PRACH_NOMA_PTC: return arrived ? u->preambleTxCounter : -1;
    case PRACH_NOMA_RETX: return arrived ? u->maxRarCounter : -1;
    case PRACH_NOMA_MSG3FAIL: return arrived ? (int64_t)(u->failCount >> 16) : -1; /* (arithmetic shift: a negative word is undefined) */
    case PRACH_NOMA_AGE: return arrived ? E - a : -1;
    case PRACH_NOMA_STATE: return noma_state(u, cls, E);
    case PRACH_NOMA_SECTOR: return arrived ? u->preambleChange : -1;
    case PRACH_NOMA_PREAMBLE: return arrived ? u->preamble : -1;
    default: /* LOST: a negative sojourn or timer makes it undefined, and so does a timer beyond the sojourn */
        if (!served) return -1;
        { const int64_t sj = (int64_t)u->txTime + 6 - a; return sj < 0 || u->timer < 0 ? -1 : sj - u->timer; }
    }
}

/* what a definition needs to know about a menu */
#define MENU_MAX_CLASSES 4
typedef struct host_menu {
    int (*class_of)(const prach_ue_log *u);
    int64_t (*value)(int field, const prach_ue_log *u, int cls, int64_t a, int64_t E);
    int classes, nfields, idle;              /* every class bit; the number of fields; the idle bit */
    int nclasses, counter[MENU_MAX_CLASSES]; /* the class bits in the order of the class counters */
    int noma_c;                              /* the cfgs the menu is defined for: 1 NOMA_C only, 0 every other variant (the rest: PRACH_ERR_UNSUPPORTED) */
} host_menu;
#define NOMA_ALL_CLASSES (PRACH_NOMA_SERVED | PRACH_NOMA_PENDING | PRACH_NOMA_IDLE | PRACH_NOMA_DROPPED)
static const host_menu XTAB_MENU = {xtab_class, xtab_value, PRACH_XTAB_SERVED | PRACH_XTAB_UNSERVED | PRACH_XTAB_IDLE, PRACH_XTAB_NFIELDS, PRACH_XTAB_IDLE,
                                    3, {PRACH_XTAB_IDLE, PRACH_XTAB_SERVED, PRACH_XTAB_UNSERVED, 0}, 0};
static const host_menu NOMA_MENU = {noma_class, noma_value, NOMA_ALL_CLASSES, PRACH_NOMA_NFIELDS, PRACH_NOMA_IDLE,
                                    4, {PRACH_NOMA_IDLE, PRACH_NOMA_SERVED, PRACH_NOMA_DROPPED, PRACH_NOMA_PENDING}, 1};

/* the schedule of a cfg of the menu's variants and E = min(steps, maxTime); NULL: a status is in *rc (ARG before UNSUPPORTED before the cfg's own validity) */
static int32_t *menu_schedule(const host_menu *m, const prach_cfg *cfg, int nUE, uint64_t steps, int *nslots, int64_t *E, int *rc) {
    *rc = PRACH_ERR_ARG;
    if (!cfg) return NULL;
    if ((cfg->variant == PRACH_VARIANT_NOMA_C) != m->noma_c) { *rc = PRACH_ERR_UNSUPPORTED; return NULL; }
    if (prach_cfg_validate(cfg) != PRACH_OK || nUE != cfg->nUE) return NULL;
    *nslots = (prach_max_time(cfg) + cfg->accessTime - 1) / cfg->accessTime;
    int32_t *sched = (int32_t *)malloc(sizeof(int32_t) * (size_t)*nslots);
    if (!sched) { *rc = PRACH_ERR_INTERNAL; return NULL; }
    prach_arrival_schedule(cfg, sched, *nslots, NULL);
    *E = steps < (uint64_t)prach_max_time(cfg) ? (int64_t)steps : (int64_t)prach_max_time(cfg);
    *rc = PRACH_OK;
    return sched;
}

/* the three judges of a spec */
static int menu_axis_ok(const host_menu *m, int field, int width, int bins) {
    return field >= 0 && field < m->nfields && width >= 1 && bins >= 1 && bins <= PRACH_XTAB_MAX_BINS;
}
static int menu_census_spec_ok(const host_menu *m, const prach_xtab_spec *s) {
    return s && s->who > 0 && (s->who & ~m->classes) == 0 && menu_axis_ok(m, s->row_field, s->row_width, s->row_bins) &&
           menu_axis_ok(m, s->col_field, s->col_width, s->col_bins) && s->reserved[0] == 0 && s->reserved[1] == 0;
}
static int menu_columns_spec_ok(const host_menu *m, const prach_columns_spec *s) {
    if (!s || s->ncols < 1 || s->ncols > PRACH_COL_MAX || s->reserved[0] || s->reserved[1] || s->reserved[2]) return 0;
    for (int c = 0; c < s->ncols; c++) {
        const int f = s->field[c];
        if (!((f >= 0 && f < m->nfields) || (f >= PRACH_COL_RAW && f < PRACH_COL_RAW + 16))) return 0;
    }
    return 1;
}
static int menu_pick_spec_ok(const host_menu *m, const prach_pick_spec *s) {
    if (!s || s->who <= 0 || (s->who & ~m->classes) != 0 || s->nclauses < 0 || s->nclauses > PRACH_PICK_MAX_CLAUSES || s->k < 1 || s->k > PRACH_PICK_MAX_K ||
        s->reserved != 0 || s->key_field < 0 || s->key_field >= m->nfields) return 0;
    if (s->order != PRACH_PICK_BY_INDEX && s->order != PRACH_PICK_LARGEST && s->order != PRACH_PICK_SMALLEST) return 0;
    if (s->order == PRACH_PICK_BY_INDEX && s->key_field != 0) return 0; /* (field 0 is ONE in both menus) */
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++) {
        const prach_pick_clause *q = &s->clause[c];
        if (c < s->nclauses ? (q->field < 0 || q->field >= m->nfields || q->lo < 0 || q->lo > q->hi) : (q->field || q->lo || q->hi)) return 0;
    }
    return 1;
}
/* (the engine judges a spec with these too: csrc/prach_device.h) */
static int census_shape(const host_menu *m, const void *spec, size_t words[]) {
    const prach_xtab_spec *s = (const prach_xtab_spec *)spec;
    if (!menu_census_spec_ok(m, s)) return 0;
    words[0] = ((size_t)s->row_bins + 1) * ((size_t)s->col_bins + 1);
    return 1;
}
static int xtab_shape(const void *spec, size_t words[]) { return census_shape(&XTAB_MENU, spec, words); }
static int noma_census_shape(const void *spec, size_t words[]) { return census_shape(&NOMA_MENU, spec, words); }
int prach_internal_noma_census_spec_ok(const prach_xtab_spec *s) { return menu_census_spec_ok(&NOMA_MENU, s); }
int prach_internal_columns_spec_ok(const prach_columns_spec *s) { return menu_columns_spec_ok(&XTAB_MENU, s); }
int prach_internal_noma_columns_spec_ok(const prach_columns_spec *s) { return menu_columns_spec_ok(&NOMA_MENU, s); }
int prach_internal_pick_spec_ok(const prach_pick_spec *s) { return menu_pick_spec_ok(&XTAB_MENU, s); }
int prach_internal_noma_pick_spec_ok(const prach_pick_spec *s) { return menu_pick_spec_ok(&NOMA_MENU, s); }

/* THE DEFINITION of the census (prach_xtab_accumulate_logs, prach_noma_census_accumulate_logs).  The two group structs differ in their class counters, so the
 * loop reaches a group through pointers to its words */
typedef struct census_group {
    uint64_t *trials, *ues, *cls[MENU_MAX_CLASSES], *selected, *binned, *undefined, *row_sum, *col_sum;
    int64_t *row_max, *col_max;
} census_group;
static int menu_census_accumulate(const host_menu *m, const prach_xtab_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE,
                                  const census_group *x, uint64_t *cells) {
    if (!menu_census_spec_ok(m, s) || !cfg || !cells || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    int nslots = 0, rc;
    int64_t E = 0;
    int32_t *sched = menu_schedule(m, cfg, nUE, steps, &nslots, &E, &rc);
    if (!sched) return rc;
    if (*x->trials == 0 && *x->binned == 0) *x->row_max = *x->col_max = -1; /* (a zero-filled group is an empty one) */
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        const int64_t a = (int64_t)cfg->accessTime * slot;
        const int cls = m->class_of(&ue[i]);
        for (int k = 0; k < m->nclasses; k++)
            if (cls == m->counter[k]) (*x->cls[k])++;
        if (!(cls & s->who)) continue;
        (*x->selected)++;
        const int64_t rv = m->value(s->row_field, &ue[i], cls, a, E), cv = m->value(s->col_field, &ue[i], cls, a, E);
        if (rv < 0 || cv < 0) { (*x->undefined)++; continue; }
        const int64_t rq = rv / s->row_width, cq = cv / s->col_width;
        const size_t r = rq < s->row_bins ? (size_t)rq : (size_t)s->row_bins, c = cq < s->col_bins ? (size_t)cq : (size_t)s->col_bins;
        cells[r * ((size_t)s->col_bins + 1) + c]++;
        (*x->binned)++;
        *x->row_sum += (uint64_t)rv;
        *x->col_sum += (uint64_t)cv;
        if (rv > *x->row_max) *x->row_max = rv;
        if (cv > *x->col_max) *x->col_max = cv;
    }
    free(sched);
    (*x->trials)++;
    *x->ues += (uint64_t)nUE;
    return PRACH_OK;
}
int prach_xtab_accumulate_logs(const prach_xtab_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_xtab *x, uint64_t *cells) {
    if (!x) return PRACH_ERR_ARG;
    const census_group g = {&x->trials, &x->ues, {&x->idle, &x->served, &x->unserved, NULL}, &x->selected, &x->binned, &x->undefined, &x->row_sum, &x->col_sum,
                            &x->row_max, &x->col_max};
    return menu_census_accumulate(&XTAB_MENU, s, cfg, steps, ue, nUE, &g, cells);
}
int prach_noma_census_accumulate_logs(const prach_xtab_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_noma_census *x,
                                      uint64_t *cells) {
    if (!x) return PRACH_ERR_ARG;
    const census_group g = {&x->trials, &x->ues, {&x->idle, &x->served, &x->dropped, &x->pending}, &x->selected, &x->binned, &x->undefined, &x->row_sum, &x->col_sum,
                            &x->row_max, &x->col_max};
    return menu_census_accumulate(&NOMA_MENU, s, cfg, steps, ue, nUE, &g, cells);
}

/* THE DEFINITION of the columns (prach_columns_from_logs, prach_noma_columns_from_logs) */
static int menu_columns(const host_menu *m, const prach_columns_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, int32_t *out,
                        uint64_t stride) {
    if (!menu_columns_spec_ok(m, s) || !cfg || !out || nUE < 0 || (nUE > 0 && !ue) || stride < (uint64_t)nUE) return PRACH_ERR_ARG;
    int nslots = 0, rc;
    int64_t E = 0;
    int32_t *sched = menu_schedule(m, cfg, nUE, steps, &nslots, &E, &rc);
    if (!sched) return rc;
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        const int64_t a = (int64_t)cfg->accessTime * slot;
        const int cls = m->class_of(&ue[i]);
        for (int c = 0; c < s->ncols; c++) {
            const int f = s->field[c];
            int32_t v;
            if (f >= PRACH_COL_RAW) v = ((const int32_t *)&ue[i])[f - PRACH_COL_RAW]; /* the log word as it is */
            else {
                const int64_t x = m->value(f, &ue[i], cls, a, E);
                v = x < 0 ? -1 : (int32_t)x; /* a negative value is UNDEFINED */
            }
            out[(size_t)c * (size_t)stride + (size_t)i] = v;
        }
    }
    free(sched);
    return PRACH_OK;
}
int prach_columns_from_logs(const prach_columns_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, int32_t *out, uint64_t stride) {
    return menu_columns(&XTAB_MENU, s, cfg, steps, ue, nUE, out, stride);
}
int prach_noma_columns_from_logs(const prach_columns_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, int32_t *out, uint64_t stride) {
    return menu_columns(&NOMA_MENU, s, cfg, steps, ue, nUE, out, stride);
}

/* ---- NOMA.c's timeline per trial group and sector (prach_run_trials_noma_timeline): THE DEFINITION, CSV ---- */

static int noma_timeline_shape(const void *spec, size_t words[]) {
    const prach_noma_timeline_spec *s = (const prach_noma_timeline_spec *)spec;
    return s ? series_shape(s->bins, s->bin_ms, PRACH_TIMELINE_MAX_BINS, 6, 6, words) : 0;
}

/* THE DEFINITION (include/prach.h), on the menu's own class and values: nothing of a log is refused, what the menu calls undefined is counted */
int prach_noma_timeline_accumulate_logs(const prach_noma_timeline_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE,
                                        prach_noma_timeline *t, uint64_t *const series[6]) {
    if (!spec_ok(noma_timeline_shape, s) || !cfg || !t || !series || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    for (int q = 0; q < 6; q++) if (!series[q]) return PRACH_ERR_ARG;
    int nslots = 0, rc;
    int64_t E = 0;
    int32_t *sched = menu_schedule(&NOMA_MENU, cfg, nUE, steps, &nslots, &E, &rc);
    if (!sched) return rc;
    if (t->trials == 0 && t->served == 0) t->done_max = -1; /* (a zero-filled group is an empty one) */
    uint64_t *const arrivals = series[0], *const served = series[1], *const dropped = series[2], *const sojourn_sum = series[3], *const timer_sum = series[4],
                    *const done = series[5];
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        const int64_t a = (int64_t)cfg->accessTime * slot;
        const prach_ue_log *u = &ue[i];
        const int cls = noma_class(u);
        if (cls == PRACH_NOMA_IDLE) { t->idle++; continue; }
        if (cls == PRACH_NOMA_SERVED) t->served++;
        else if (cls == PRACH_NOMA_DROPPED) t->dropped++;
        else t->pending++;
        const int64_t sec = noma_value(PRACH_NOMA_SECTOR, u, cls, a, E), sj = noma_value(PRACH_NOMA_SOJOURN, u, cls, a, E),
                      tm = noma_value(PRACH_NOMA_TIMER, u, cls, a, E), c = noma_value(PRACH_NOMA_COMPLETION, u, cls, a, E);
        if (sec < 0 || sec > 5 || (cls == PRACH_NOMA_SERVED && (sj < 0 || tm < 0 || c < 0))) { t->undefined++; continue; }
        const int64_t ab = noma_value(PRACH_NOMA_ARRIVAL, u, cls, a, E) / s->bin_ms;
        const size_t at = (size_t)sec * (size_t)s->bins + (size_t)ab;
        if (ab < s->bins) arrivals[at]++;
        else t->arrival_overflow++;
        if (cls == PRACH_NOMA_DROPPED && ab < s->bins) dropped[at]++;
        if (cls != PRACH_NOMA_SERVED) continue;
        const int64_t db = c / s->bin_ms;
        t->sojourn_sum += (uint64_t)sj;
        t->timer_sum += (uint64_t)tm;
        t->restarted += noma_value(PRACH_NOMA_LOST, u, cls, a, E) > 0;
        if (c > t->done_max) t->done_max = c;
        if (ab < s->bins) { served[at]++; sojourn_sum[at] += (uint64_t)sj; timer_sum[at] += (uint64_t)tm; }
        if (db < s->bins) done[(size_t)sec * (size_t)s->bins + (size_t)db]++;
        else t->done_overflow++;
    }
    free(sched);
    t->trials++;
    t->ues += (uint64_t)nUE;
    return PRACH_OK;
}

static size_t noma_timeline_csv(const void *spec, const void *group, const uint64_t *const series[], const char *label, char *buf, size_t cap) {
    static const char *const names[6] = {"arrivals", "served", "dropped", "sojourn_sum", "timer_sum", "done"};
    static const series_lines lines = {names, 6, 6, 2, {{0, 0, offsetof(prach_noma_timeline, arrival_overflow)}, {5, 5, offsetof(prach_noma_timeline, done_overflow)}}};
    const prach_noma_timeline_spec *s = (const prach_noma_timeline_spec *)spec;
    return series_csv(&lines, s->bins, s->bin_ms, group, series, label, buf, cap);
}

/* ---- NOMA.c's near-far profile per trial group, sector and gain level (prach_run_trials_noma_gain): the level, THE DEFINITION, CSV ---- */

/* floor(1000.0 * lgain): ONE IEEE product (no contraction: there is nothing to contract with), floor towards minus infinity */
int32_t prach_noma_gain_level(double lgain) {
    const double p = 1000.0 * lgain;
    if (!isfinite(p) || fabs(p) >= 1073741824.0) return PRACH_NOMA_GAIN_NO_LEVEL;
    return (int32_t)floor(p);
}

int prach_noma_gain_levels(const prach_cfg *cfg, int32_t *level) {
    if (!cfg || !level) return PRACH_ERR_ARG;
    if (cfg->variant != PRACH_VARIANT_NOMA_C || cfg->rng_mode == PRACH_RNG_GLIBC) return PRACH_ERR_UNSUPPORTED;
    if (prach_cfg_validate(cfg) != PRACH_OK) return PRACH_ERR_ARG;
    const size_t n = (size_t)(cfg->nUE > 0 ? cfg->nUE : 1);
    int32_t *pre = (int32_t *)malloc(4 * n), *sec = (int32_t *)malloc(4 * n);
    uint32_t *nd = (uint32_t *)malloc(4 * n);
    double *gn = (double *)malloc(8 * n), *lg = (double *)malloc(8 * n);
    int rc = pre && sec && nd && gn && lg ? prach_noma_activation_table(cfg, pre, sec, gn, lg, nd) : PRACH_ERR_INTERNAL;
    for (int i = 0; rc == PRACH_OK && i < cfg->nUE; i++) level[i] = prach_noma_gain_level(lg[i]);
    free(pre); free(sec); free(nd); free(gn); free(lg);
    return rc;
}

static int noma_gain_shape(const void *spec, size_t words[]) {
    const prach_noma_gain_spec *s = (const prach_noma_gain_spec *)spec;
    if (!s || s->bins < 1 || s->bins > PRACH_NOMA_GAIN_MAX_BINS || s->width < 1) return 0;
    for (int q = 0; q < PRACH_NOMA_GAIN_SERIES; q++) words[q] = 6 * (size_t)s->bins;
    return PRACH_NOMA_GAIN_SERIES;
}

/* THE DEFINITION (include/prach.h), on the menu's own class and values and the levels as given */
int prach_noma_gain_accumulate_levels(const prach_noma_gain_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, const int32_t *level,
                                      prach_noma_gain *g, uint64_t *const series[6]) {
    if (!spec_ok(noma_gain_shape, s) || !cfg || !g || !series || nUE < 0 || (nUE > 0 && (!ue || !level))) return PRACH_ERR_ARG;
    for (int q = 0; q < 6; q++) if (!series[q]) return PRACH_ERR_ARG;
    int nslots = 0, rc;
    int64_t E = 0;
    int32_t *sched = menu_schedule(&NOMA_MENU, cfg, nUE, steps, &nslots, &E, &rc);
    if (!sched) return rc;
    if (g->defined == 0) g->level_max = g->neg_level_max = -1; /* (a zero-filled group is an empty one) */
    uint64_t *const arrived = series[0], *const served = series[1], *const dropped = series[2], *const sojourn_sum = series[3], *const lost_sum = series[4],
                    *const ptc_sum = series[5];
    const int64_t lo = s->lo, hi = (int64_t)s->lo + (int64_t)s->bins * (int64_t)s->width;
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        const int64_t a = (int64_t)cfg->accessTime * slot;
        const prach_ue_log *u = &ue[i];
        const int cls = noma_class(u);
        if (cls == PRACH_NOMA_IDLE) { g->idle++; continue; }
        if (cls == PRACH_NOMA_SERVED) g->served++;
        else if (cls == PRACH_NOMA_DROPPED) g->dropped++;
        else g->pending++;
        const int64_t sec = noma_value(PRACH_NOMA_SECTOR, u, cls, a, E), sj = noma_value(PRACH_NOMA_SOJOURN, u, cls, a, E),
                      lost = noma_value(PRACH_NOMA_LOST, u, cls, a, E), ptc = noma_value(PRACH_NOMA_PTC, u, cls, a, E), L = level[i];
        if (sec < 0 || sec > 5 || L == PRACH_NOMA_GAIN_NO_LEVEL || (cls == PRACH_NOMA_SERVED && (sj < 0 || lost < 0 || ptc < 0))) { g->undefined++; continue; }
        if (g->defined++ == 0 || L > g->level_max) g->level_max = L;
        if (g->defined == 1 || -L > g->neg_level_max) g->neg_level_max = -L;
        const int in = L >= lo && L < hi;
        const size_t at = in ? (size_t)sec * (size_t)s->bins + (size_t)((L - lo) / s->width) : 0;
        if (L < lo) g->below++;
        else if (!in) g->above++;
        else arrived[at]++;
        if (cls == PRACH_NOMA_DROPPED && in) dropped[at]++;
        if (cls != PRACH_NOMA_SERVED) continue;
        g->sojourn_sum += (uint64_t)sj;
        g->lost_sum += (uint64_t)lost;
        g->ptc_sum += (uint64_t)ptc;
        g->restarted += lost > 0;
        if (in) { served[at]++; sojourn_sum[at] += (uint64_t)sj; lost_sum[at] += (uint64_t)lost; ptc_sum[at] += (uint64_t)ptc; }
    }
    free(sched);
    g->trials++;
    g->ues += (uint64_t)nUE;
    return PRACH_OK;
}

int prach_noma_gain_accumulate_logs(const prach_noma_gain_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_noma_gain *g,
                                    uint64_t *const series[6]) {
    if (!spec_ok(noma_gain_shape, s) || !cfg || !g || !series || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    for (int q = 0; q < 6; q++) if (!series[q]) return PRACH_ERR_ARG;
    if (cfg->variant != PRACH_VARIANT_NOMA_C || cfg->rng_mode == PRACH_RNG_GLIBC) return PRACH_ERR_UNSUPPORTED;
    if (prach_cfg_validate(cfg) != PRACH_OK || nUE != cfg->nUE) return PRACH_ERR_ARG;
    int32_t *level = (int32_t *)malloc(4 * (size_t)(nUE > 0 ? nUE : 1));
    if (!level) return PRACH_ERR_INTERNAL;
    int rc = prach_noma_gain_levels(cfg, level);
    if (rc == PRACH_OK) rc = prach_noma_gain_accumulate_levels(s, cfg, steps, ue, nUE, level, g, series);
    free(level);
    return rc;
}

static size_t noma_gain_csv(const void *spec, const void *group, const uint64_t *const series[], const char *label, char *buf, size_t cap) {
    static const char *const names[6] = {"arrived", "served", "dropped", "sojourn_sum", "lost_sum", "ptc_sum"};
    const prach_noma_gain_spec *s = (const prach_noma_gain_spec *)spec;
    const prach_noma_gain *g = (const prach_noma_gain *)group;
    size_t off = 0;
    for (int q = 0; q < 6; q++) {
        if (q == 0 && g->below) CSV_EMIT("%.200s,%s,all,below,%llu\n", label, names[0], (unsigned long long)g->below);
        for (int b = 0; b < s->bins; b++) {
            const long long edge = (long long)s->lo + (long long)b * s->width;
            uint64_t all = 0;
            for (int c = 0; c < 6; c++) {
                const uint64_t v = series[q][(size_t)c * (size_t)s->bins + (size_t)b];
                all += v;
                if (v) CSV_EMIT("%.200s,%s,%d,%lld,%llu\n", label, names[q], c, edge, (unsigned long long)v);
            }
            if (all) CSV_EMIT("%.200s,%s,all,%lld,%llu\n", label, names[q], edge, (unsigned long long)all);
        }
        if (q == 0 && g->above) CSV_EMIT("%.200s,%s,all,above,%llu\n", label, names[0], (unsigned long long)g->above);
    }
    return csv_end(buf, cap, off);
}

/* THE DEFINITION of the pick (prach_pick_from_logs, prach_noma_pick_from_logs): every match is listed, the list is sorted, the first k are the rows */
typedef struct pick_cand { int64_t key; int32_t i, arrival; } pick_cand;
static int cmp_pick_desc(const void *a, const void *b) { /* descending key, equal keys in ascending UE index */
    const pick_cand *x = (const pick_cand *)a, *y = (const pick_cand *)b;
    return x->key != y->key ? (x->key < y->key) - (x->key > y->key) : (x->i > y->i) - (x->i < y->i);
}
static int cmp_pick_asc(const void *a, const void *b) {
    const pick_cand *x = (const pick_cand *)a, *y = (const pick_cand *)b;
    return x->key != y->key ? (x->key > y->key) - (x->key < y->key) : (x->i > y->i) - (x->i < y->i);
}
static int menu_pick(const host_menu *m, const prach_pick_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_pick *hdr,
                     prach_pick_row *rows) {
    if (!menu_pick_spec_ok(m, s) || !cfg || !hdr || !rows || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    int nslots = 0, rc;
    int64_t E = 0;
    int32_t *sched = menu_schedule(m, cfg, nUE, steps, &nslots, &E, &rc);
    if (!sched) return rc;
    pick_cand *cand = (pick_cand *)malloc(sizeof(pick_cand) * (size_t)(nUE > 0 ? nUE : 1));
    if (!cand) { free(sched); return PRACH_ERR_INTERNAL; }
    const int keyed = s->order != PRACH_PICK_BY_INDEX;
    prach_pick h;
    memset(&h, 0, sizeof h);
    h.status = PRACH_OK; h.nUE = nUE; h.threshold = -1;
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        const int64_t a = (int64_t)cfg->accessTime * slot;
        const int cls = m->class_of(&ue[i]);
        if (!(cls & s->who)) continue;
        h.selected++;
        int fails = 0, undef = 0;
        for (int c = 0; c < s->nclauses; c++) {
            const int64_t v = m->value(s->clause[c].field, &ue[i], cls, a, E);
            if (v < 0) undef = 1;
            else if (v < s->clause[c].lo || v > s->clause[c].hi) fails = 1;
        }
        const int64_t key = keyed ? m->value(s->key_field, &ue[i], cls, a, E) : 0;
        if (key < 0) undef = 1;
        if (fails) continue;
        if (undef) { h.undefined++; continue; }
        cand[h.matched++] = (pick_cand){key, i, cls == m->idle ? -1 : (int32_t)a};
    }
    if (keyed) qsort(cand, (size_t)h.matched, sizeof(pick_cand), s->order == PRACH_PICK_LARGEST ? cmp_pick_desc : cmp_pick_asc);
    h.stored = h.matched < s->k ? h.matched : s->k;
    memset(rows, 0, sizeof(prach_pick_row) * (size_t)s->k);
    for (int r = 0; r < h.stored; r++) {
        rows[r].log = ue[cand[r].i];
        rows[r].arrival = cand[r].arrival;
        rows[r].key = (int32_t)cand[r].key;
    }
    if (keyed && h.stored > 0) {
        h.threshold = rows[h.stored - 1].key;
        for (int r = h.stored; r < h.matched && cand[r].key == cand[h.stored - 1].key; r++) h.ties_left_out++;
    }
    free(sched);
    free(cand);
    *hdr = h;
    return PRACH_OK;
}
int prach_pick_from_logs(const prach_pick_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_pick *hdr, prach_pick_row *rows) {
    return menu_pick(&XTAB_MENU, s, cfg, steps, ue, nUE, hdr, rows);
}
int prach_noma_pick_from_logs(const prach_pick_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE, prach_pick *hdr, prach_pick_row *rows) {
    return menu_pick(&NOMA_MENU, s, cfg, steps, ue, nUE, hdr, rows);
}

/* ---- outcome cross-tabulation per trial group (prach_run_trials_xtab) and the NOMA census (prach_run_trials_noma_census): quantile, CSV ---------- */

int64_t prach_xtab_quantile(const prach_xtab_spec *s, const uint64_t *cells, int row, double q) {
    if (!spec_ok(xtab_shape, s) || !cells || row < -1 || row > s->row_bins || !(q >= 0.0) || q > 1.0) return -1;
    const int r0 = row < 0 ? 0 : row, r1 = row < 0 ? s->row_bins + 1 : row + 1;
    const size_t W = (size_t)s->col_bins + 1;
    uint64_t n = 0;
    for (int r = r0; r < r1; r++)
        for (size_t c = 0; c < W; c++) n += cells[(size_t)r * W + c];
    if (n == 0) return -1;
    uint64_t rank = (uint64_t)ceil(q * (double)n);
    if (rank < 1) rank = 1;
    if (rank > n) rank = n;
    uint64_t cum = 0;
    for (int c = 0; c < s->col_bins; c++) {
        for (int r = r0; r < r1; r++) cum += cells[(size_t)r * W + (size_t)c];
        if (cum >= rank) return (int64_t)c * s->col_width;
    }
    return -1; /* in the overflow column */
}

/* the lines of both: only widths, bin counts and `undefined` enter them */
static size_t census_lines(const prach_xtab_spec *s, uint64_t undefined, const uint64_t *cells, const char *label, char *buf, size_t cap) {
    size_t off = 0;
    const size_t W = (size_t)s->col_bins + 1;
    for (int r = 0; r <= s->row_bins; r++)
        for (int c = 0; c <= s->col_bins; c++) {
            const uint64_t v = cells[(size_t)r * W + (size_t)c];
            if (!v) continue;
            char re[24], ce[24];
            if (r < s->row_bins) snprintf(re, sizeof re, "%lld", (long long)r * s->row_width); else strcpy(re, "overflow");
            if (c < s->col_bins) snprintf(ce, sizeof ce, "%lld", (long long)c * s->col_width); else strcpy(ce, "overflow");
            CSV_EMIT("%.200s,%s,%s,%llu\n", label, re, ce, (unsigned long long)v);
        }
    if (undefined) CSV_EMIT("%.200s,undefined,,%llu\n", label, (unsigned long long)undefined);
    return csv_end(buf, cap, off);
}
static size_t xtab_csv(const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap) {
    return census_lines((const prach_xtab_spec *)spec, ((const prach_xtab *)group)->undefined, arrays[0], label, buf, cap);
}
static size_t noma_census_csv(const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap) {
    return census_lines((const prach_xtab_spec *)spec, ((const prach_noma_census *)group)->undefined, arrays[0], label, buf, cap);
}

/* ---- the grouped kinds (prach_grouped.h): one row each, the generic shape, merge and CSV over the rows, and the public functions as wrappers ---- */

#define GROUPED_ROW(SPEC, GROUP, GUARD, MAXIMA, RESERVED_WORDS, TRIALS, SHAPE, FORMAT) \
    {sizeof(SPEC), sizeof(GROUP), (int)(sizeof(GROUP) / 8) - (MAXIMA), MAXIMA, (int)(offsetof(GROUP, GUARD) / 8), SHAPE, offsetof(SPEC, ngroups), offsetof(SPEC, reserved), \
     RESERVED_WORDS, TRIALS, FORMAT}
/* in the order of the enumerators PRACH_G_*:  spec, group struct, guard counter, maxima, reserved words, trials, shape, CSV */
static const prach_grouped_row GROUPED[PRACH_G_KINDS] = {
    GROUPED_ROW(prach_dist_spec, prach_dist, success, 1, 1, PRACH_G_TRIALS_ANY, dist_shape, dist_csv),
    GROUPED_ROW(prach_timeline_spec, prach_timeline, success, 1, 1, PRACH_G_TRIALS_NOT_NOMA_C, timeline_shape, timeline_csv),
    GROUPED_ROW(prach_sojourn_spec, prach_sojourn, success, 1, 1, PRACH_G_TRIALS_NOT_NOMA_C, sojourn_shape, sojourn_csv),
    GROUPED_ROW(prach_trace_spec, prach_trace, subframes, 1, 1, PRACH_G_TRIALS_NOT_NOMA_C, trace_shape, trace_csv),
    GROUPED_ROW(prach_xtab_spec, prach_xtab, binned, 2, 2, PRACH_G_TRIALS_NOT_NOMA_C, xtab_shape, xtab_csv),
    GROUPED_ROW(prach_xtab_spec, prach_noma_census, binned, 2, 2, PRACH_G_TRIALS_NOMA_C_PHILOX, noma_census_shape, noma_census_csv),
    GROUPED_ROW(prach_noma_trace_spec, prach_noma_trace, slots, 1, 1, PRACH_G_TRIALS_NOMA_C_PHILOX, noma_trace_shape, noma_trace_csv),
    GROUPED_ROW(prach_noma_timeline_spec, prach_noma_timeline, served, 1, 1, PRACH_G_TRIALS_NOMA_C_PHILOX, noma_timeline_shape, noma_timeline_csv),
};
/* ... and of the enumerators from PRACH_G_MORE on */
static const prach_grouped_row GROUPED_MORE[PRACH_G_MORE_END - PRACH_G_MORE] = {
    GROUPED_ROW(prach_noma_gain_spec, prach_noma_gain, defined, 2, 1, PRACH_G_TRIALS_NOMA_C_PHILOX, noma_gain_shape, noma_gain_csv),
};

const prach_grouped_row *prach_internal_grouped_row(int kind) {
    return kind >= 0 && kind < PRACH_G_KINDS ? &GROUPED[kind] : kind >= PRACH_G_MORE && kind < PRACH_G_MORE_END ? &GROUPED_MORE[kind - PRACH_G_MORE] : NULL;
}

int prach_internal_grouped_shape(int kind, const void *spec, size_t words[PRACH_G_MAX_ARRAYS]) {
    const prach_grouped_row *k = prach_internal_grouped_row(kind);
    return k ? k->shape(spec, words) : 0;
}

/* the shape of a call on one group: 0 unless the spec is good and the group and every array are there */
static int grouped_args(int kind, const void *spec, const void *group, const uint64_t *const arrays[], size_t words[PRACH_G_MAX_ARRAYS]) {
    const int na = prach_internal_grouped_shape(kind, spec, words);
    if (!na || !group || !arrays) return 0;
    for (int q = 0; q < na; q++) if (!arrays[q]) return 0;
    return na;
}

void prach_internal_grouped_merge(int kind, const void *spec, void *into, uint64_t *const into_arrays[], const void *from, const uint64_t *const from_arrays[]) {
    size_t words[PRACH_G_MAX_ARRAYS];
    const int na = grouped_args(kind, spec, into, (const uint64_t *const *)into_arrays, words);
    if (!na || !grouped_args(kind, spec, from, from_arrays, words)) return;
    const prach_grouped_row *k = prach_internal_grouped_row(kind);
    uint64_t *const a = (uint64_t *)into;
    const uint64_t *const b = (const uint64_t *)from;
    int64_t *const amax = (int64_t *)into + k->counters;
    const int64_t *const bmax = (const int64_t *)from + k->counters;
    for (int m = 0; m < k->maxima; m++) { /* (a maximum only counts if the guard counter is non-zero: judged before the counters are added; -1 where neither
                                             counts, and a side that does not count never wins: the gain profile's maxima may lie below -1) */
        const int64_t x = amax[m], y = bmax[m];
        amax[m] = !a[k->guard] ? (b[k->guard] ? y : -1) : !b[k->guard] || x > y ? x : y;
    }
    for (int c = 0; c < k->counters; c++) a[c] += b[c];
    for (int q = 0; q < na; q++)
        for (size_t i = 0; i < words[q]; i++) into_arrays[q][i] += from_arrays[q][i];
}

size_t prach_internal_grouped_format_csv(int kind, const void *spec, const void *group, const uint64_t *const arrays[], const char *label, char *buf, size_t cap) {
    size_t words[PRACH_G_MAX_ARRAYS];
    if (!grouped_args(kind, spec, group, arrays, words) || !label) return 0;
    return prach_internal_grouped_row(kind)->format(spec, group, arrays, label, buf, cap);
}

void prach_dist_merge(const prach_dist_spec *s, prach_dist *into, uint64_t *dh_into, uint64_t *ph_into, const prach_dist *from, const uint64_t *dh_from,
                      const uint64_t *ph_from) {
    uint64_t *const a[2] = {dh_into, ph_into};
    const uint64_t *const b[2] = {dh_from, ph_from};
    prach_internal_grouped_merge(PRACH_G_DIST, s, into, a, from, b);
}
size_t prach_dist_format_csv(const prach_dist_spec *s, const prach_dist *d, const uint64_t *delay_hist, const uint64_t *ptc_hist, const char *label, char *buf,
                             size_t cap) {
    const uint64_t *const a[2] = {delay_hist, ptc_hist};
    return prach_internal_grouped_format_csv(PRACH_G_DIST, s, d, a, label, buf, cap);
}
void prach_timeline_merge(const prach_timeline_spec *s, prach_timeline *into, uint64_t *const into_series[5], const prach_timeline *from,
                          const uint64_t *const from_series[5]) {
    prach_internal_grouped_merge(PRACH_G_TIMELINE, s, into, into_series, from, from_series);
}
size_t prach_timeline_format_csv(const prach_timeline_spec *s, const prach_timeline *t, const uint64_t *const series[5], const char *label, char *buf, size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_TIMELINE, s, t, series, label, buf, cap);
}
void prach_sojourn_merge(const prach_sojourn_spec *s, prach_sojourn *into, uint64_t *hist_into, uint64_t *arrived_into, uint64_t *overflow_into,
                         const prach_sojourn *from, const uint64_t *hist_from, const uint64_t *arrived_from, const uint64_t *overflow_from) {
    uint64_t *const a[3] = {hist_into, arrived_into, overflow_into};
    const uint64_t *const b[3] = {hist_from, arrived_from, overflow_from};
    prach_internal_grouped_merge(PRACH_G_SOJOURN, s, into, a, from, b);
}
size_t prach_sojourn_format_csv(const prach_sojourn_spec *s, const prach_sojourn *j, const uint64_t *hist, const uint64_t *row_arrived,
                                const uint64_t *row_delay_overflow, const char *label, char *buf, size_t cap) {
    const uint64_t *const a[3] = {hist, row_arrived, row_delay_overflow};
    return prach_internal_grouped_format_csv(PRACH_G_SOJOURN, s, j, a, label, buf, cap);
}
void prach_trace_merge(const prach_trace_spec *s, prach_trace *into, uint64_t *const into_series[4], const prach_trace *from, const uint64_t *const from_series[4]) {
    prach_internal_grouped_merge(PRACH_G_TRACE, s, into, into_series, from, from_series);
}
size_t prach_trace_format_csv(const prach_trace_spec *s, const prach_trace *t, const uint64_t *const series[4], const char *label, char *buf, size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_TRACE, s, t, series, label, buf, cap);
}
void prach_xtab_merge(const prach_xtab_spec *s, prach_xtab *into, uint64_t *cells_into, const prach_xtab *from, const uint64_t *cells_from) {
    prach_internal_grouped_merge(PRACH_G_XTAB, s, into, &cells_into, from, &cells_from);
}
size_t prach_xtab_format_csv(const prach_xtab_spec *s, const prach_xtab *x, const uint64_t *cells, const char *label, char *buf, size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_XTAB, s, x, &cells, label, buf, cap);
}
void prach_noma_census_merge(const prach_xtab_spec *s, prach_noma_census *into, uint64_t *cells_into, const prach_noma_census *from, const uint64_t *cells_from) {
    prach_internal_grouped_merge(PRACH_G_NOMA_CENSUS, s, into, &cells_into, from, &cells_from);
}
size_t prach_noma_census_format_csv(const prach_xtab_spec *s, const prach_noma_census *x, const uint64_t *cells, const char *label, char *buf, size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_NOMA_CENSUS, s, x, &cells, label, buf, cap);
}
void prach_noma_trace_merge(const prach_noma_trace_spec *s, prach_noma_trace *into, uint64_t *const into_series[6], const prach_noma_trace *from,
                            const uint64_t *const from_series[6]) {
    prach_internal_grouped_merge(PRACH_G_NOMA_TRACE, s, into, into_series, from, from_series);
}
size_t prach_noma_trace_format_csv(const prach_noma_trace_spec *s, const prach_noma_trace *t, const uint64_t *const series[6], const char *label, char *buf, size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_NOMA_TRACE, s, t, series, label, buf, cap);
}
void prach_noma_timeline_merge(const prach_noma_timeline_spec *s, prach_noma_timeline *into, uint64_t *const into_series[6], const prach_noma_timeline *from,
                               const uint64_t *const from_series[6]) {
    prach_internal_grouped_merge(PRACH_G_NOMA_TIMELINE, s, into, into_series, from, from_series);
}
size_t prach_noma_timeline_format_csv(const prach_noma_timeline_spec *s, const prach_noma_timeline *t, const uint64_t *const series[6], const char *label, char *buf,
                                      size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_NOMA_TIMELINE, s, t, series, label, buf, cap);
}

void prach_noma_gain_merge(const prach_noma_gain_spec *s, prach_noma_gain *into, uint64_t *const into_series[6], const prach_noma_gain *from,
                           const uint64_t *const from_series[6]) {
    prach_internal_grouped_merge(PRACH_G_NOMA_GAIN, s, into, into_series, from, from_series);
}
size_t prach_noma_gain_format_csv(const prach_noma_gain_spec *s, const prach_noma_gain *g, const uint64_t *const series[6], const char *label, char *buf, size_t cap) {
    return prach_internal_grouped_format_csv(PRACH_G_NOMA_GAIN, s, g, series, label, buf, cap);
}

/* ---- picks: the UEs behind a count, per trial (prach_run_trials_pick, prach_run_trials_noma_pick): CSV ---- */

size_t prach_pick_format_csv(const prach_pick_spec *s, const prach_pick *h, const prach_pick_row *rows, const char *label, int trial, uint64_t seed, char *buf,
                             size_t cap) {
    if (!prach_internal_pick_spec_ok(s) || !h || !rows || !label || h->stored < 0 || h->stored > s->k) return 0;
    size_t off = 0;
    CSV_EMIT("%.200s,%d,%llu,%d,header,%d,%d,%d,%d,%d,%d,%d\n", label, trial, (unsigned long long)seed, h->nUE, h->status, h->selected, h->matched, h->stored, h->undefined,
             h->threshold, h->ties_left_out);
    for (int r = 0; r < h->stored; r++) {
        const prach_ue_log *u = &rows[r].log;
        CSV_EMIT("%.200s,%d,%llu,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n", label, trial, (unsigned long long)seed, h->nUE, r, rows[r].key, rows[r].arrival,
                 u->idx, u->timer, u->active, u->txTime, u->firstTxTime, u->secondTxTime, u->nowBackoff, u->preamble, u->preambleChange, u->rarWindow, u->maxRarCounter,
                 u->preambleTxCounter, u->msg2Flag, u->connectionRequest, u->msg4Flag, u->failCount);
    }
    return csv_end(buf, cap, off);
}

size_t prach_noma_pick_format_csv(const prach_pick_spec *s, const prach_pick *h, const prach_pick_row *rows, const char *label, int trial, uint64_t seed, char *buf,
                                  size_t cap) {
    if (!prach_internal_noma_pick_spec_ok(s)) return 0;
    /* the pick's lines: only k enters them */
    prach_pick_spec t;
    memset(&t, 0, sizeof t);
    t.who = PRACH_XTAB_SERVED; t.order = PRACH_PICK_BY_INDEX; t.key_field = PRACH_XTAB_ONE; t.k = s->k;
    return prach_pick_format_csv(&t, h, rows, label, trial, seed, buf, cap);
}

/* ---- the NOMA summary: one row per trial over named fields of the NOMA menu (prach_run_trials_noma_summary) ---- */

/* (the engine judges a spec with this too: csrc/prach_device.h) */
int prach_internal_noma_summary_spec_ok(const prach_noma_summary_spec *s) {
    if (!s || s->who <= 0 || (s->who & ~NOMA_ALL_CLASSES) != 0 || s->nfields < 1 || s->nfields > PRACH_NOMA_SUMMARY_MAX_FIELDS || s->nq < 1 ||
        s->nq > PRACH_SUMMARY_MAX_Q || s->reserved[0] || s->reserved[1]) return 0;
    for (int x = 0; x < PRACH_NOMA_SUMMARY_MAX_FIELDS; x++)
        if (x < s->nfields ? (s->field[x] < 0 || s->field[x] >= PRACH_NOMA_NFIELDS) : s->field[x] != 0) return 0;
    for (int l = 0; l < s->nq; l++)
        if (s->permille[l] < 1 || s->permille[l] > 1000) return 0;
    return 1;
}

static void noma_summary_row_clear(prach_noma_trial_summary *row, int status, int nUE) {
    memset(row, 0, sizeof(*row));
    row->status = status;
    row->nUE = nUE;
    for (int x = 0; x < PRACH_NOMA_SUMMARY_MAX_FIELDS; x++) {
        row->max[x] = -1;
        for (int l = 0; l < PRACH_SUMMARY_MAX_Q; l++) row->q[x][l] = -1;
    }
}

static int cmp_i64(const void *a, const void *b) {
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return (x > y) - (x < y);
}

/* THE DEFINITION (include/prach.h): the defined values of every named field over the selected UEs are sorted, a level is the value at its integer rank */
int prach_noma_summary_from_logs(const prach_noma_summary_spec *s, const prach_cfg *cfg, uint64_t steps, const prach_ue_log *ue, int nUE,
                                 prach_noma_trial_summary *row) {
    if (!prach_internal_noma_summary_spec_ok(s) || !cfg || !row || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    int nslots = 0, rc;
    int64_t E = 0;
    int32_t *sched = menu_schedule(&NOMA_MENU, cfg, nUE, steps, &nslots, &E, &rc);
    if (!sched) return rc;
    int64_t *val = (int64_t *)malloc(sizeof(int64_t) * PRACH_NOMA_SUMMARY_MAX_FIELDS * (size_t)(nUE > 0 ? nUE : 1));
    if (!val) { free(sched); return PRACH_ERR_INTERNAL; }
    prach_noma_trial_summary r;
    noma_summary_row_clear(&r, PRACH_OK, nUE);
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        const int64_t a = (int64_t)cfg->accessTime * slot;
        const int cls = noma_class(&ue[i]);
        if (cls == PRACH_NOMA_IDLE) r.idle++;
        else if (cls == PRACH_NOMA_SERVED) r.served++;
        else if (cls == PRACH_NOMA_DROPPED) r.dropped++;
        else r.pending++;
        r.restarted += noma_value(PRACH_NOMA_LOST, &ue[i], cls, a, E) > 0; /* (defined for the served only) */
        if (!(cls & s->who)) continue;
        r.selected++;
        for (int x = 0; x < s->nfields; x++) {
            const int64_t v = noma_value(s->field[x], &ue[i], cls, a, E);
            if (v < 0) continue; /* UNDEFINED */
            val[(size_t)x * (size_t)nUE + (size_t)r.n[x]++] = v;
            r.sum[x] += v;
        }
    }
    for (int x = 0; x < s->nfields; x++) {
        const int64_t n = r.n[x];
        if (n == 0) continue;
        int64_t *const v = val + (size_t)x * (size_t)nUE;
        qsort(v, (size_t)n, sizeof(int64_t), cmp_i64);
        r.max[x] = (int32_t)v[n - 1];
        for (int l = 0; l < s->nq; l++) {
            int64_t rank = (n * (int64_t)s->permille[l] + 999) / 1000;
            if (rank < 1) rank = 1;
            r.q[x][l] = (int32_t)v[rank - 1];
        }
    }
    free(sched);
    free(val);
    *row = r;
    return PRACH_OK;
}

#define NOMA_SUMMARY_FIXED_METRICS 4
/* metric m of a row; returns 0 where the row has no such value */
static int noma_summary_metric(const prach_noma_summary_spec *s, const prach_noma_trial_summary *r, int m, double *x) {
    if (r->status != PRACH_OK) return 0;
    if (m < 3) { *x = (double)(m == 0 ? r->served : m == 1 ? r->dropped : r->pending) / (double)r->nUE; return r->nUE > 0; }
    if (m == 3) { *x = (double)r->restarted / (double)r->served; return r->served > 0; }
    const int f = (m - NOMA_SUMMARY_FIXED_METRICS) / (1 + s->nq), j = (m - NOMA_SUMMARY_FIXED_METRICS) % (1 + s->nq);
    if (r->n[f] == 0) return 0;
    *x = j == 0 ? (double)r->sum[f] / (double)r->n[f] : (double)r->q[f][j - 1];
    return 1;
}

int prach_noma_summary_stats(const prach_noma_summary_spec *s, const prach_noma_trial_summary *rows, int n, const int32_t *group, int ngroups, prach_stat *out) {
    if (!prach_internal_noma_summary_spec_ok(s) || n < 0 || (n > 0 && !rows) || ngroups < 1 || !out || (!group && ngroups != 1)) return PRACH_ERR_ARG;
    if (group)
        for (int k = 0; k < n; k++)
            if (group[k] < 0 || group[k] >= ngroups) return PRACH_ERR_ARG;
    const int nm = NOMA_SUMMARY_FIXED_METRICS + s->nfields * (1 + s->nq);
    memset(out, 0, sizeof(prach_stat) * (size_t)ngroups * (size_t)nm);
    for (int m = 0; m < nm; m++) {
        double x;
        for (int k = 0; k < n; k++) { /* pass 1: count, sum, extremes */
            if (!noma_summary_metric(s, &rows[k], m, &x)) continue;
            prach_stat *const o = &out[(size_t)(group ? group[k] : 0) * (size_t)nm + (size_t)m];
            if (o->n == 0 || x < o->min) o->min = x;
            if (o->n == 0 || x > o->max) o->max = x;
            o->n++;
            o->mean += x;
        }
        for (int g = 0; g < ngroups; g++) {
            prach_stat *const o = &out[(size_t)g * (size_t)nm + (size_t)m];
            if (o->n) o->mean /= (double)o->n;
        }
        for (int k = 0; k < n; k++) { /* pass 2: squared deviations from the mean */
            if (!noma_summary_metric(s, &rows[k], m, &x)) continue;
            prach_stat *const o = &out[(size_t)(group ? group[k] : 0) * (size_t)nm + (size_t)m];
            o->sd += (x - o->mean) * (x - o->mean);
        }
        for (int g = 0; g < ngroups; g++) {
            prach_stat *const o = &out[(size_t)g * (size_t)nm + (size_t)m];
            o->sd = o->n > 1 ? sqrt(o->sd / (double)(o->n - 1)) : 0.0;
            o->sem = o->n > 1 ? o->sd / sqrt((double)o->n) : 0.0;
        }
    }
    return PRACH_OK;
}

size_t prach_noma_summary_format_csv(const prach_noma_summary_spec *s, const prach_stat *st, const char *label, char *buf, size_t cap) {
    static const char *const fixed[NOMA_SUMMARY_FIXED_METRICS] = {"served_ratio", "dropped_ratio", "pending_ratio", "restart_ratio"};
    static const char *const names[PRACH_NOMA_NFIELDS] = {"one", "arrival", "sojourn", "completion", "timer", "ptc", "retx", "msg3fail", "age", "state", "sector", "preamble", "lost"};
    if (!prach_internal_noma_summary_spec_ok(s) || !st || !label) return 0;
    size_t off = 0;
    const int nm = NOMA_SUMMARY_FIXED_METRICS + s->nfields * (1 + s->nq);
    for (int m = 0; m < nm; m++) {
        char name[32];
        const int f = (m - NOMA_SUMMARY_FIXED_METRICS) / (1 + s->nq), j = (m - NOMA_SUMMARY_FIXED_METRICS) % (1 + s->nq);
        if (m < NOMA_SUMMARY_FIXED_METRICS) snprintf(name, sizeof name, "%s", fixed[m]);
        else if (j == 0) snprintf(name, sizeof name, "%s_mean", names[s->field[f]]);
        else snprintf(name, sizeof name, "%s_p%d", names[s->field[f]], s->permille[j - 1]);
        CSV_EMIT("%.200s,%s,%llu,%.9g,%.9g,%.9g,%.9g,%.9g\n", label, name, (unsigned long long)st[m].n, st[m].mean, st[m].sd, st[m].sem, st[m].min, st[m].max);
    }
    return csv_end(buf, cap, off);
}

/* ---- per-trial summaries: exact order statistics and the spread across trials (prach_run_trials_summary) ---- */

static int summary_spec_ok(const prach_summary_spec *s) {
    if (!s || s->nq < 1 || s->nq > PRACH_SUMMARY_MAX_Q || s->reserved[0] || s->reserved[1] || s->reserved[2]) return 0;
    for (int l = 0; l < s->nq; l++)
        if (s->permille[l] < 1 || s->permille[l] > 1000) return 0;
    return 1;
}

int prach_summary_max_value(void) { return 65535; }

static void summary_row_clear(prach_trial_summary *row, int status, int nUE) {
    memset(row, 0, sizeof(*row));
    row->status = status;
    row->nUE = nUE;
    row->sojourn_max = row->timer_max = row->ptc_max = -1;
    for (int x = 0; x < 3; x++)
        for (int l = 0; l < PRACH_SUMMARY_MAX_Q; l++) row->q[x][l] = -1;
}

static int cmp_i32(const void *a, const void *b) {
    const int32_t x = *(const int32_t *)a, y = *(const int32_t *)b;
    return (x > y) - (x < y);
}

/* THE DEFINITION (include/prach.h): the three quantities of the successful UEs are sorted, a level is the value at its integer rank */
int prach_summary_from_logs(const prach_summary_spec *s, const prach_cfg *cfg, const prach_ue_log *ue, int nUE, prach_trial_summary *row) {
    if (!summary_spec_ok(s) || !cfg || !row || nUE < 0 || (nUE > 0 && !ue)) return PRACH_ERR_ARG;
    if (cfg->variant == PRACH_VARIANT_NOMA_C) return PRACH_ERR_UNSUPPORTED;
    if (prach_cfg_validate(cfg) != PRACH_OK || nUE != cfg->nUE) return PRACH_ERR_ARG;
    const int nslots = (prach_max_time(cfg) + cfg->accessTime - 1) / cfg->accessTime;
    int32_t *sched = (int32_t *)malloc(sizeof(int32_t) * (size_t)nslots);
    int32_t *val = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)(nUE > 0 ? nUE : 1));
    if (!sched || !val) { free(sched); free(val); return PRACH_ERR_INTERNAL; }
    prach_arrival_schedule(cfg, sched, nslots, NULL);
    prach_trial_summary r;
    summary_row_clear(&r, PRACH_OK, nUE);
    int32_t *const vx[3] = {val, val + nUE, val + 2 * (size_t)nUE};
    int slot = 0; /* UEs are activated in index order: the slot of UE i is not before the slot of UE i - 1 */
    for (int i = 0; i < nUE; i++) {
        while (slot < nslots && sched[slot] <= i) slot++;
        if (ue[i].active == -1) continue; /* not arrived */
        r.arrived++;
        if (ue[i].msg4Flag != 1) continue;
        const int64_t a = (int64_t)cfg->accessTime * slot, c = (int64_t)ue[i].txTime + 6;
        if (ue[i].timer < 0 || c < a) { free(sched); free(val); return PRACH_ERR_ARG; } /* (*row is untouched) */
        const int n = r.success++;
        r.restarted += c - ue[i].timer != a;
        vx[0][n] = (int32_t)(c - a); vx[1][n] = ue[i].timer; vx[2][n] = ue[i].preambleTxCounter;
        r.sojourn_sum += c - a; r.timer_sum += ue[i].timer; r.ptc_sum += ue[i].preambleTxCounter;
    }
    const int64_t n = r.success;
    if (n > 0) {
        int32_t *const mx[3] = {&r.sojourn_max, &r.timer_max, &r.ptc_max};
        for (int x = 0; x < 3; x++) {
            qsort(vx[x], (size_t)n, sizeof(int32_t), cmp_i32);
            *mx[x] = vx[x][n - 1];
            for (int l = 0; l < s->nq; l++) {
                int64_t rank = (n * (int64_t)s->permille[l] + 999) / 1000;
                if (rank < 1) rank = 1;
                r.q[x][l] = vx[x][rank - 1];
            }
        }
    }
    free(sched);
    free(val);
    *row = r;
    return PRACH_OK;
}

#define SUMMARY_FIXED_METRICS 5
/* metric m of a row; returns 0 where the row has no such value */
static int summary_metric(const prach_summary_spec *s, const prach_trial_summary *r, int m, double *x) {
    if (r->status != PRACH_OK) return 0;
    if (m == 0) { *x = (double)r->success / (double)r->nUE; return r->nUE > 0; }
    if (r->success == 0) return 0;
    const double n = (double)r->success;
    if (m == 1) *x = (double)r->restarted / n;
    else if (m == 2) *x = (double)r->sojourn_sum / n;
    else if (m == 3) *x = (double)r->timer_sum / n;
    else if (m == 4) *x = (double)r->ptc_sum / n;
    else *x = (double)r->q[(m - SUMMARY_FIXED_METRICS) / s->nq][(m - SUMMARY_FIXED_METRICS) % s->nq];
    return 1;
}

int prach_summary_stats(const prach_summary_spec *s, const prach_trial_summary *rows, int n, const int32_t *group, int ngroups, prach_stat *out) {
    if (!summary_spec_ok(s) || n < 0 || (n > 0 && !rows) || ngroups < 1 || !out || (!group && ngroups != 1)) return PRACH_ERR_ARG;
    if (group)
        for (int k = 0; k < n; k++)
            if (group[k] < 0 || group[k] >= ngroups) return PRACH_ERR_ARG;
    const int nm = SUMMARY_FIXED_METRICS + 3 * s->nq;
    memset(out, 0, sizeof(prach_stat) * (size_t)ngroups * (size_t)nm);
    for (int m = 0; m < nm; m++) {
        double x;
        for (int k = 0; k < n; k++) { /* pass 1: count, sum, extremes */
            if (!summary_metric(s, &rows[k], m, &x)) continue;
            prach_stat *const o = &out[(size_t)(group ? group[k] : 0) * (size_t)nm + (size_t)m];
            if (o->n == 0 || x < o->min) o->min = x;
            if (o->n == 0 || x > o->max) o->max = x;
            o->n++;
            o->mean += x;
        }
        for (int g = 0; g < ngroups; g++) {
            prach_stat *const o = &out[(size_t)g * (size_t)nm + (size_t)m];
            if (o->n) o->mean /= (double)o->n;
        }
        for (int k = 0; k < n; k++) { /* pass 2: squared deviations from the mean */
            if (!summary_metric(s, &rows[k], m, &x)) continue;
            prach_stat *const o = &out[(size_t)(group ? group[k] : 0) * (size_t)nm + (size_t)m];
            o->sd += (x - o->mean) * (x - o->mean);
        }
        for (int g = 0; g < ngroups; g++) {
            prach_stat *const o = &out[(size_t)g * (size_t)nm + (size_t)m];
            o->sd = o->n > 1 ? sqrt(o->sd / (double)(o->n - 1)) : 0.0;
            o->sem = o->n > 1 ? o->sd / sqrt((double)o->n) : 0.0;
        }
    }
    return PRACH_OK;
}

size_t prach_summary_format_csv(const prach_summary_spec *s, const prach_stat *st, const char *label, char *buf, size_t cap) {
    static const char *const fixed[SUMMARY_FIXED_METRICS] = {"success_ratio", "restart_ratio", "sojourn_mean", "timer_mean", "ptx_mean"};
    static const char *const quant[3] = {"sojourn", "timer", "ptx"};
    if (!summary_spec_ok(s) || !st || !label) return 0;
    size_t off = 0;
    const int nm = SUMMARY_FIXED_METRICS + 3 * s->nq;
    for (int m = 0; m < nm; m++) {
        char name[32];
        if (m < SUMMARY_FIXED_METRICS) snprintf(name, sizeof name, "%s", fixed[m]);
        else snprintf(name, sizeof name, "%s_p%d", quant[(m - SUMMARY_FIXED_METRICS) / s->nq], s->permille[(m - SUMMARY_FIXED_METRICS) % s->nq]);
        CSV_EMIT("%.200s,%s,%llu,%.9g,%.9g,%.9g,%.9g,%.9g\n", label, name, (unsigned long long)st[m].n, st[m].mean, st[m].sd, st[m].sem, st[m].min, st[m].max);
    }
    return csv_end(buf, cap, off);
}
