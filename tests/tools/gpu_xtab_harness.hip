// tests/tools/gpu_xtab_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::xtab_kernel launched directly, through launch_xtab_kernel, on buffers of this
// program's own, filled from a case file that tests/tools/xtab_cases.py writes: per-UE state no simulation leaves behind.  One launch per process; every
// per-job array sits at a 256-byte-aligned device offset, as in the engine's arena (the kernel's 16-byte loads rely on it).  The kernel's source file is
// compiled into this program as it is; no product entry point is involved.
//
// usage: gpu_xtab_harness CASE RESULT SCHEME     exit code 0 = launched, synchronised and written; anything else is an error (message on stderr)
//        gpu_xtab_harness --constants            the kernel's compile-time constants, one "NAME value" per line (no device needed)
//
// CASE (int32, little endian):   header[16] = magic, 3, njobs, who, row_field, row_width, row_bins, col_field, col_width, col_bins, ngroups, 0 ...
//                                jobs[njobs][8] = nUE, group, 0, aT, nslots, E, 0, 0
//                                per job, in job order: logs[nUE][16], then sched[nslots]
// RESULT (uint64):               header[4] = magic, 3, scheme, workgroups
//                                cells[ngroups][row_bins + 1][col_bins + 1], scalars[ngroups][XT_SCALARS]
#include "../../5g-nr-randomaccess_amd/csrc/prach_xtab.hip"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int MAGIC = 0x52445543;
constexpr long long MAX_UE_TOTAL = 1ll << 24, MAX_JOBS = 1 << 16, MAX_GROUPS = 64, MAX_OUT_WORDS = 1ll << 26;

#define CHK(call)                                                                                              \
    do {                                                                                                       \
        const hipError_t rc_ = (call);                                                                         \
        if (rc_ != hipSuccess) {                                                                               \
            fprintf(stderr, "gpu_xtab_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                          \
        }                                                                                                      \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_xtab_harness: %s\n", what);
    return 3;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct JobRow { int nUE, group, form, aT, nslots, E, pad[2]; };

} // namespace

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("TL_TILE %d\nTL_THREADS %d\nXT_WINDOW_WORDS %d\nXT_COPY_WORDS %d\nXT_SCHED_CAP %d\nXT_SCALARS %d\n", TL_TILE, TL_THREADS, XT_WINDOW_WORDS, XT_COPY_WORDS,
               XT_SCHED_CAP, XT_SCALARS);
        return 0;
    }
    if (argc != 4) return fail("usage: gpu_xtab_harness CASE RESULT SCHEME | --constants");
    const int scheme = atoi(argv[3]);

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
    const int kind = w[1], njobs = w[2], ngroups = w[10];
    const XtabAxes ax{w[3], w[4], w[5], w[6], w[7], w[8], w[9]};
    if (w[0] != MAGIC || kind != 3) return fail("case file: bad header");
    if (njobs < 1 || njobs > MAX_JOBS || ngroups < 1 || ngroups > MAX_GROUPS || ax.row_width < 1 || ax.col_width < 1) return fail("case file: njobs / ngroups / widths out of range");
    if (ax.row_bins < 1 || ax.row_bins > PRACH_XTAB_MAX_BINS || ax.col_bins < 1 || ax.col_bins > PRACH_XTAB_MAX_BINS) return fail("case file: bin counts out of range");
    if (ax.who < 1 || ax.who > 7 || ax.row_field < 0 || ax.row_field >= PRACH_XTAB_NFIELDS || ax.col_field < 0 || ax.col_field >= PRACH_XTAB_NFIELDS) return fail("case file: who / fields out of range");
    if (scheme < 0 || scheme > 1) return fail("scheme out of range");
    if (w.size() < 16 + 8 * (size_t)njobs) return fail("case file: job table cut short");
    const JobRow *const jr = reinterpret_cast<const JobRow *>(w.data() + 16);
    const size_t ng = (size_t)ngroups, cells = ng * ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const size_t out_words = cells + ng * XT_SCALARS;
    if ((long long)out_words > MAX_OUT_WORDS) return fail("case file: outputs too large");

    // ---- every array of every job: checked against the file, placed at a 256-byte-aligned arena offset
    struct Place { size_t src_a, n_a, dst_a, src_b, n_b, dst_b; }; // in ints (src, n) and bytes (dst)
    std::vector<Place> pl((size_t)njobs);
    size_t src = 16 + 8 * (size_t)njobs, arena = 0;
    long long total_ue = 0;
    int wgs = 0;
    for (int j = 0; j < njobs; j++) {
        const JobRow &r = jr[j];
        if (r.nUE < 1 || r.group < 0 || r.group >= ngroups) return fail("job: nUE / group out of range");
        total_ue += r.nUE;
        if (total_ue > MAX_UE_TOTAL) return fail("case file: too many UEs");
        if (r.aT < 1 || r.nslots < 1 || r.nslots > (1 << 20) || (long long)r.aT * r.nslots > INT_MAX || r.E < 0) return fail("job: aT / nslots / E out of range");
        const size_t na = 16 * (size_t)r.nUE, nb = (size_t)r.nslots;
        wgs += (r.nUE + TL_TILE - 1) / TL_TILE;
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

    // ---- device: arena, job table, zeroed outputs; ONE launch
    unsigned char *A = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&A), arena));
    CHK(hipMemcpy(A, stage.data(), arena, hipMemcpyHostToDevice));
    unsigned long long *O = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&O), 8 * out_words));
    CHK(hipMemset(O, 0, 8 * out_words));
    int wg0 = 0;
    std::vector<TimelineJob> jobs((size_t)njobs);
    for (int j = 0; j < njobs; j++) {
        jobs[(size_t)j] = TimelineJob{reinterpret_cast<const int4 *>(A + pl[(size_t)j].dst_a), reinterpret_cast<const int *>(A + pl[(size_t)j].dst_b), jr[j].nUE, jr[j].group, wg0,
                                      jr[j].aT, jr[j].nslots, jr[j].E};
        wg0 += (jr[j].nUE + TL_TILE - 1) / TL_TILE;
    }
    TimelineJob *tj = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&tj), sizeof(TimelineJob) * jobs.size()));
    CHK(hipMemcpy(tj, jobs.data(), sizeof(TimelineJob) * jobs.size(), hipMemcpyHostToDevice));
    CHK(launch_xtab_kernel(tj, njobs, wgs, ax, scheme, XtabOut{O, O + cells}, nullptr));
    CHK(hipDeviceSynchronize());

    std::vector<unsigned long long> res(4 + out_words);
    res[0] = (unsigned long long)MAGIC; res[1] = 3ull; res[2] = (unsigned long long)scheme; res[3] = (unsigned long long)wgs;
    CHK(hipMemcpy(res.data() + 4, O, 8 * out_words, hipMemcpyDeviceToHost));
    FILE *g = fopen(argv[2], "wb");
    if (!g) return fail("cannot open the result file");
    const size_t put = fwrite(res.data(), 8, res.size(), g);
    if (fclose(g) != 0 || put != res.size()) return fail("result file: short write");
    return 0;
}
