// tests/tools/gpu_pick_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::pick_kernel launched directly, through launch_pick_kernel, on buffers of this
// program's own, filled from a case file that tests/tools/pick_cases.py writes: per-UE state no simulation leaves behind.  One launch per process; every
// per-job array sits at a 256-byte-aligned device offset, as in the engine's arena (the kernel's 16-byte loads and stores rely on it).  The kernel's source
// file is compiled into this program as it is; no product entry point is involved (the spec check of prach_host.c is restated below: the host C file is
// not part of this program).
//
// usage: gpu_pick_harness CASE RESULT THREADS    exit code 0 = launched, synchronised and written; anything else is an error (message on stderr)
//        gpu_pick_harness --constants            the kernel's compile-time constants, one "NAME value" per line (no device needed)
//
// CASE (int32, little endian):   header[32] = magic, 4, njobs, who, nclauses, clause[4][3] = field, lo, hi, order, key_field, k, 0 ...
//                                jobs[njobs][8] = nUE, trial, 0, aT, nslots, E, 0, 0
//                                per job, in job order: logs[nUE][16], then sched[nslots]
// RESULT (uint64):               header[4] = magic, 4, threads, njobs
//                                scalars[njobs][PK_SCALARS], then rows[njobs][k][PK_ROW_WORDS]: as the kernel leaves them (what it does not write stays at the
//                                fill pattern 0x5A: the rows behind `stored`, and everything of a trial no job names)
#include "../../5g-nr-randomaccess_amd/csrc/prach_pick.hip"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int prach_internal_pick_spec_ok(const prach_pick_spec *s) { // prach_host.c's, for this program
    if (!s || s->who <= 0 || (s->who & ~7) != 0 || s->nclauses < 0 || s->nclauses > PRACH_PICK_MAX_CLAUSES || s->k < 1 || s->k > PRACH_PICK_MAX_K || s->reserved != 0 ||
        s->key_field < 0 || s->key_field >= PRACH_XTAB_NFIELDS || s->order < 0 || s->order > 2 || (s->order == PRACH_PICK_BY_INDEX && s->key_field != 0)) return 0;
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++) {
        const prach_pick_clause *q = &s->clause[c];
        if (c < s->nclauses ? (q->field < 0 || q->field >= PRACH_XTAB_NFIELDS || q->lo < 0 || q->lo > q->hi) : (q->field || q->lo || q->hi)) return 0;
    }
    return 1;
}

namespace {

constexpr int MAGIC = 0x52445543;
constexpr long long MAX_UE_TOTAL = 1ll << 24, MAX_JOBS = 1 << 12;

#define CHK(call)                                                                                            \
    do {                                                                                                     \
        const hipError_t rc_ = (call);                                                                       \
        if (rc_ != hipSuccess) {                                                                             \
            fprintf(stderr, "gpu_pick_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                        \
        }                                                                                                    \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_pick_harness: %s\n", what);
    return 3;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct JobRow { int nUE, group, form, aT, nslots, E, pad[2]; };

} // namespace

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("PK_ROW_WORDS %d\nPK_SCALARS %d\nPK_MAX_KEY %d\nPK_SCHED_CAP %d\nPK_COARSE %d\nPK_FINE %d\nPRACH_PICK_MAX_K %d\nPRACH_PICK_MAX_CLAUSES %d\nTL_MAX_SOJOURN %d\n", PK_ROW_WORDS,
               PK_SCALARS, PK_MAX_KEY, PK_SCHED_CAP, PK_COARSE, PK_FINE, PRACH_PICK_MAX_K, PRACH_PICK_MAX_CLAUSES, TL_MAX_SOJOURN);
        return 0;
    }
    if (argc != 4) return fail("usage: gpu_pick_harness CASE RESULT THREADS | --constants");
    const int threads = atoi(argv[3]);
    if (threads != 512 && threads != 1024) return fail("threads: 512 or 1024");

    // ---- the case file, whole
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    fseek(f, 0, SEEK_END);
    const long fbytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fbytes < 128 || fbytes % 4) { fclose(f); return fail("case file: bad length"); }
    std::vector<int> w((size_t)fbytes / 4);
    const size_t got = fread(w.data(), 4, w.size(), f);
    fclose(f);
    if (got != w.size()) return fail("case file: short read");
    const int kind = w[1], njobs = w[2];
    if (w[0] != MAGIC || kind != 4) return fail("case file: bad header");
    prach_pick_spec sp{};
    sp.who = w[3]; sp.nclauses = w[4];
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++) sp.clause[c] = prach_pick_clause{w[5 + 3 * c], w[6 + 3 * c], w[7 + 3 * c]};
    sp.order = w[17]; sp.key_field = w[18]; sp.k = w[19];
    if (njobs < 1 || njobs > MAX_JOBS || !prach_internal_pick_spec_ok(&sp)) return fail("case file: njobs out of range or a bad spec"); // (k bounds every row store)
    if (w.size() < 32 + 8 * (size_t)njobs) return fail("case file: job table cut short");
    const JobRow *const jr = reinterpret_cast<const JobRow *>(w.data() + 32);
    const size_t sc_words = (size_t)njobs * PK_SCALARS, row_words = (size_t)njobs * (size_t)sp.k * PK_ROW_WORDS;

    // ---- every array of every job: checked against the file, placed at a 256-byte-aligned arena offset
    struct Place { size_t src_a, n_a, dst_a, src_b, n_b, dst_b; }; // in ints (src, n) and bytes (dst)
    std::vector<Place> pl((size_t)njobs);
    size_t src = 32 + 8 * (size_t)njobs, arena = 0;
    long long total_ue = 0;
    int max_slots = 0;
    for (int j = 0; j < njobs; j++) {
        const JobRow &r = jr[j];
        if (r.nUE < 1 || r.group < 0 || r.group >= njobs) return fail("job: nUE / trial out of range"); // (a trial index is the offset of the stores)
        total_ue += r.nUE;
        if (total_ue > MAX_UE_TOTAL) return fail("case file: too many UEs");
        if (r.aT < 1 || r.nslots < 1 || r.nslots > (1 << 20) || (long long)r.aT * r.nslots > INT_MAX) return fail("job: aT / nslots out of range");
        if (r.nslots > max_slots) max_slots = r.nslots;
        const size_t na = 16 * (size_t)r.nUE, nb = (size_t)r.nslots;
        if (src + na + nb > w.size()) return fail("case file: arrays cut short");
        pl[(size_t)j] = Place{src, na, arena, src + na, nb, align256(arena + 4 * na)};
        arena = align256(pl[(size_t)j].dst_b + 4 * nb);
        src += na + nb;
        const int *const s = w.data() + pl[(size_t)j].src_b; // a schedule is non-decreasing and counts UEs of this trial: the kernel's searches assume it
        for (int q = 0; q < r.nslots; q++)
            if (s[q] < 0 || s[q] > r.nUE || (q && s[q] < s[q - 1])) return fail("job: schedule not a non-decreasing count of UEs");
    }
    if (src != w.size()) return fail("case file: trailing data");

    std::vector<unsigned char> stage(arena, 0xA5); // (the gaps between arrays hold a pattern, never zeros)
    for (int j = 0; j < njobs; j++) {
        const Place &p = pl[(size_t)j];
        memcpy(stage.data() + p.dst_a, w.data() + p.src_a, 4 * p.n_a);
        memcpy(stage.data() + p.dst_b, w.data() + p.src_b, 4 * p.n_b);
    }

    // ---- device: arena, job table, outputs filled with a pattern; ONE launch
    unsigned char *A = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&A), arena));
    CHK(hipMemcpy(A, stage.data(), arena, hipMemcpyHostToDevice));
    unsigned long long *O = nullptr; // scalars, then rows (the rows start at a multiple of 64 bytes)
    CHK(hipMalloc(reinterpret_cast<void **>(&O), 8 * (sc_words + row_words)));
    CHK(hipMemset(O, 0x5A, 8 * (sc_words + row_words)));
    std::vector<TimelineJob> jobs((size_t)njobs);
    for (int j = 0; j < njobs; j++)
        jobs[(size_t)j] = TimelineJob{reinterpret_cast<const int4 *>(A + pl[(size_t)j].dst_a), reinterpret_cast<const int *>(A + pl[(size_t)j].dst_b), jr[j].nUE, jr[j].group, j,
                                      jr[j].aT, jr[j].nslots, jr[j].E};
    TimelineJob *tj = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&tj), sizeof(TimelineJob) * jobs.size()));
    CHK(hipMemcpy(tj, jobs.data(), sizeof(TimelineJob) * jobs.size(), hipMemcpyHostToDevice));
    CHK(launch_pick_kernel(tj, njobs, sp, threads, max_slots < PK_SCHED_CAP ? max_slots : PK_SCHED_CAP, O + sc_words, O, nullptr)); // (the engine's staging rule)
    CHK(hipDeviceSynchronize());

    std::vector<unsigned long long> res(4 + sc_words + row_words);
    res[0] = (unsigned long long)MAGIC; res[1] = 4ull; res[2] = (unsigned long long)threads; res[3] = (unsigned long long)njobs;
    CHK(hipMemcpy(res.data() + 4, O, 8 * (sc_words + row_words), hipMemcpyDeviceToHost));
    FILE *g = fopen(argv[2], "wb");
    if (!g) return fail("cannot open the result file");
    const size_t put = fwrite(res.data(), 8, res.size(), g);
    if (fclose(g) != 0 || put != res.size()) return fail("result file: short write");
    return 0;
}
