// tests/tools/gpu_summary_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::summary_kernel launched directly, through launch_summary_kernel, on buffers
// of this program's own, filled from a case file that tests/tools/summary_cases.py writes: per-UE state no simulation leaves behind.  One launch per
// process; every per-job array sits at a 256-byte-aligned device offset, as in the engine's arena (the kernel's 16-byte loads rely on it).  The kernel's
// source file is compiled into this program as it is; no product entry point is involved.
//
// usage: gpu_summary_harness CASE RESULT THREADS    exit code 0 = launched, synchronised and written; anything else is an error (message on stderr)
//        gpu_summary_harness --constants            the kernel's compile-time constants, one "NAME value" per line (no device needed)
//
// CASE (int32, little endian):   header[16] = magic, 3, njobs, nq, permille[8], 0 ...
//                                jobs[njobs][8] = nUE, row, 0, aT, nslots, 0, 0, 0
//                                per job, in job order: logs[nUE][16], then sched[nslots]
// RESULT (uint64):               header[4] = magic, 3, threads, njobs
//                                rows[njobs][SM_WORDS]: the kernel's rows as they are (a row no job names stays at the fill pattern and fails the comparison)
#include "../../5g-nr-randomaccess_amd/csrc/prach_summary.hip"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int MAGIC = 0x52445543;
constexpr long long MAX_UE_TOTAL = 1ll << 24, MAX_JOBS = 1 << 16;

#define CHK(call)                                                                                              \
    do {                                                                                                       \
        const hipError_t rc_ = (call);                                                                         \
        if (rc_ != hipSuccess) {                                                                               \
            fprintf(stderr, "gpu_summary_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                          \
        }                                                                                                      \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_summary_harness: %s\n", what);
    return 3;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct JobRow { int nUE, group, form, aT, nslots, pad[3]; };

} // namespace

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("SM_WORDS %d\nSM_MAX_VALUE %d\nSM_SCHED_CAP %d\nSM_COARSE %d\nSM_FINE %d\nPRACH_SUMMARY_MAX_Q %d\nTL_MAX_SOJOURN %d\n", SM_WORDS, SM_MAX_VALUE, SM_SCHED_CAP,
               SM_COARSE, SM_FINE, PRACH_SUMMARY_MAX_Q, TL_MAX_SOJOURN);
        return 0;
    }
    if (argc != 4) return fail("usage: gpu_summary_harness CASE RESULT THREADS | --constants");
    const int threads = atoi(argv[3]);
    if (threads != 512 && threads != 1024) return fail("threads: 512 or 1024");

    // ---- the case file, whole
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    fseek(f, 0, SEEK_END);
    const long fbytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fbytes < 64 || fbytes % 4) { fclose(f); return fail("case file: bad length"); }
    std::vector<int> w((size_t)fbytes / 4);
    const size_t got = fread(w.data(), 4, w.size(), f);
    fclose(f);
    if (got != w.size()) return fail("case file: short read");
    const int kind = w[1], njobs = w[2];
    if (w[0] != MAGIC || kind != 3) return fail("case file: bad header");
    SummaryLevels lv{};
    lv.nq = w[3];
    if (njobs < 1 || njobs > MAX_JOBS || lv.nq < 1 || lv.nq > PRACH_SUMMARY_MAX_Q) return fail("case file: njobs / nq out of range");
    for (int l = 0; l < lv.nq; l++) {
        lv.permille[l] = w[4 + l];
        if (lv.permille[l] < 1 || lv.permille[l] > 1000) return fail("case file: level out of range");
    }
    if (w.size() < 16 + 8 * (size_t)njobs) return fail("case file: job table cut short");
    const JobRow *const jr = reinterpret_cast<const JobRow *>(w.data() + 16);
    const size_t out_words = (size_t)njobs * SM_WORDS;

    // ---- every array of every job: checked against the file, placed at a 256-byte-aligned arena offset
    struct Place { size_t src_a, n_a, dst_a, src_b, n_b, dst_b; }; // in ints (src, n) and bytes (dst)
    std::vector<Place> pl((size_t)njobs);
    size_t src = 16 + 8 * (size_t)njobs, arena = 0;
    long long total_ue = 0;
    int max_slots = 0;
    for (int j = 0; j < njobs; j++) {
        const JobRow &r = jr[j];
        if (r.nUE < 1 || r.group < 0 || r.group >= njobs) return fail("job: nUE / row out of range"); // (a row index is the offset of a store)
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

    // ---- device: arena, job table, outputs filled with a pattern (the kernel stores whole rows); ONE launch
    unsigned char *A = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&A), arena));
    CHK(hipMemcpy(A, stage.data(), arena, hipMemcpyHostToDevice));
    unsigned long long *O = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&O), 8 * out_words));
    CHK(hipMemset(O, 0x5A, 8 * out_words));
    std::vector<TimelineJob> jobs((size_t)njobs);
    for (int j = 0; j < njobs; j++)
        jobs[(size_t)j] = TimelineJob{reinterpret_cast<const int4 *>(A + pl[(size_t)j].dst_a), reinterpret_cast<const int *>(A + pl[(size_t)j].dst_b), jr[j].nUE, jr[j].group, j,
                                      jr[j].aT, jr[j].nslots, 0};
    TimelineJob *tj = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&tj), sizeof(TimelineJob) * jobs.size()));
    CHK(hipMemcpy(tj, jobs.data(), sizeof(TimelineJob) * jobs.size(), hipMemcpyHostToDevice));
    CHK(launch_summary_kernel(tj, njobs, lv, threads, max_slots < SM_SCHED_CAP ? max_slots : SM_SCHED_CAP, O, nullptr)); // (the engine's staging rule)
    CHK(hipDeviceSynchronize());

    std::vector<unsigned long long> res(4 + out_words);
    res[0] = (unsigned long long)MAGIC; res[1] = 3ull; res[2] = (unsigned long long)threads; res[3] = (unsigned long long)njobs;
    CHK(hipMemcpy(res.data() + 4, O, 8 * out_words, hipMemcpyDeviceToHost));
    FILE *g = fopen(argv[2], "wb");
    if (!g) return fail("cannot open the result file");
    const size_t put = fwrite(res.data(), 8, res.size(), g);
    if (fclose(g) != 0 || put != res.size()) return fail("result file: short write");
    return 0;
}
