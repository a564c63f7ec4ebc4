// tests/tools/gpu_noma_census_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::noma_census_kernel and prach::noma_columns_kernel launched directly,
// through their launch functions, on buffers of this program's own, filled from a case file that tests/tools/noma_census_cases.py writes: per-UE state no
// simulation leaves behind.  One launch per process; every per-job array sits at a 256-byte-aligned device offset, as in the engine's arena (the kernels'
// 16-byte loads rely on it).  The kernels' source file is compiled into this program as it is; no product entry point is involved.
//
// usage: gpu_noma_census_harness CASE RESULT census SCHEME | CASE RESULT columns     exit code 0 = launched, synchronised and written
//        gpu_noma_census_harness --constants            the kernels' compile-time constants, one "NAME value" per line (no device needed)
//
// CASE (int32, little endian):   header[32] = magic, 9, njobs, who, row_field, row_width, row_bins, col_field, col_width, col_bins, ngroups, ncols,
//                                             field[16], 0 ...
//                                jobs[njobs][8] = nUE, group, 0, aT, nslots, E, 0, 0
//                                per job, in job order: logs[nUE][16], then sched[nslots]
// RESULT census (uint64):        header[4] = magic, 9, scheme, workgroups; cells[ngroups][row_bins + 1][col_bins + 1], scalars[ngroups][NC_SCALARS]
// RESULT columns (uint64):       header[4] = magic, 10, 0, workgroups; scalars[njobs][NCL_SCALARS]; then int32 data[ncols][rows + GUARD], rows = the sum of
//                                nUE, filled with the pattern 0x7FFF7FFF before the launch (the GUARD words behind the rows of every column must keep it)
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_census.hip"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// prach_host.c's judgement of a columns spec, restated for this program (it links no product object)
extern "C" int prach_internal_noma_columns_spec_ok(const prach_columns_spec *s) {
    if (!s || s->ncols < 1 || s->ncols > PRACH_COL_MAX || s->reserved[0] || s->reserved[1] || s->reserved[2]) return 0;
    for (int c = 0; c < s->ncols; c++) {
        const int f = s->field[c];
        if (!((f >= 0 && f < PRACH_NOMA_NFIELDS) || (f >= PRACH_COL_RAW && f < PRACH_COL_RAW + 16))) return 0;
    }
    return 1;
}

namespace {

constexpr int MAGIC = 0x52445543, PATTERN = 0x7FFF7FFF, GUARD = 64;
constexpr long long MAX_UE_TOTAL = 1ll << 24, MAX_JOBS = 1 << 16, MAX_GROUPS = 64, MAX_OUT_WORDS = 1ll << 26;

#define CHK(call)                                                                                                     \
    do {                                                                                                              \
        const hipError_t rc_ = (call);                                                                                \
        if (rc_ != hipSuccess) {                                                                                      \
            fprintf(stderr, "gpu_noma_census_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                                 \
        }                                                                                                             \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_noma_census_harness: %s\n", what);
    return 3;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct JobRow { int nUE, group, form, aT, nslots, E, pad[2]; };

} // namespace

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("TL_TILE %d\nTL_THREADS %d\nXT_WINDOW_WORDS %d\nNC_COPY_WORDS %d\nTILE_SCHED_CAP %d\nNC_SCALARS %d\nNCL_SCALARS %d\n", TL_TILE, TL_THREADS, XT_WINDOW_WORDS,
               noma_census_copy_words(), TILE_SCHED_CAP, NC_SCALARS, NCL_SCALARS);
        return 0;
    }
    const bool census = argc == 5 && !strcmp(argv[3], "census"), columns = argc == 4 && !strcmp(argv[3], "columns");
    if (!census && !columns) return fail("usage: gpu_noma_census_harness CASE RESULT census SCHEME | CASE RESULT columns | --constants");
    const int scheme = census ? atoi(argv[4]) : 0;

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
    const int njobs = w[2], ngroups = w[10];
    const XtabAxes ax{w[3], w[4], w[5], w[6], w[7], w[8], w[9]};
    prach_columns_spec sp{};
    sp.ncols = w[11];
    for (int c = 0; c < PRACH_COL_MAX; c++) sp.field[c] = w[12 + c];
    if (w[0] != MAGIC || w[1] != 9) return fail("case file: bad header");
    if (njobs < 1 || njobs > MAX_JOBS || ngroups < 1 || ngroups > MAX_GROUPS || ax.row_width < 1 || ax.col_width < 1) return fail("case file: njobs / ngroups / widths out of range");
    if (ax.row_bins < 1 || ax.row_bins > PRACH_XTAB_MAX_BINS || ax.col_bins < 1 || ax.col_bins > PRACH_XTAB_MAX_BINS) return fail("case file: bin counts out of range");
    if (ax.who < 1 || ax.who > 15 || ax.row_field < 0 || ax.row_field >= PRACH_NOMA_NFIELDS || ax.col_field < 0 || ax.col_field >= PRACH_NOMA_NFIELDS) return fail("case file: who / fields out of range");
    if (columns && !prach_internal_noma_columns_spec_ok(&sp)) return fail("case file: columns out of range");
    if (scheme < 0 || scheme > 1) return fail("scheme out of range");
    if (w.size() < 32 + 8 * (size_t)njobs) return fail("case file: job table cut short");
    const JobRow *const jr = reinterpret_cast<const JobRow *>(w.data() + 32);
    const size_t ng = (size_t)ngroups, cells = ng * ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const size_t out_words = census ? cells + ng * NC_SCALARS : (size_t)njobs * NCL_SCALARS;
    if ((long long)out_words > MAX_OUT_WORDS) return fail("case file: outputs too large");

    // ---- every array of every job: checked against the file, placed at a 256-byte-aligned arena offset
    struct Place { size_t src_a, n_a, dst_a, src_b, n_b, dst_b; }; // in ints (src, n) and bytes (dst)
    std::vector<Place> pl((size_t)njobs);
    std::vector<unsigned long long> offset((size_t)njobs);
    size_t src = 32 + 8 * (size_t)njobs, arena = 0;
    long long total_ue = 0;
    int wgs = 0;
    for (int j = 0; j < njobs; j++) {
        const JobRow &r = jr[j];
        if (r.nUE < 1 || r.group < 0 || r.group >= ngroups) return fail("job: nUE / group out of range");
        offset[(size_t)j] = (unsigned long long)total_ue;
        total_ue += r.nUE;
        if (total_ue > MAX_UE_TOTAL) return fail("case file: too many UEs");
        if (r.aT < 1 || r.nslots < 1 || r.nslots > (1 << 20) || (long long)r.aT * r.nslots > INT_MAX || r.E < 0) return fail("job: aT / nslots / E out of range");
        const size_t na = 16 * (size_t)r.nUE, nb = (size_t)r.nslots;
        wgs += (r.nUE + TL_TILE - 1) / TL_TILE;
        if (src + na + nb > w.size()) return fail("case file: arrays cut short");
        pl[(size_t)j] = Place{src, na, arena, src + na, nb, align256(arena + 4 * na)};
        arena = align256(pl[(size_t)j].dst_b + 4 * nb);
        src += na + nb;
        const int *const s = w.data() + pl[(size_t)j].src_b; // a schedule is non-decreasing and counts UEs of this trial: the kernels' searches assume it
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

    // ---- device: arena, job table, zeroed counters, patterned columns; ONE launch
    unsigned char *A = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&A), arena));
    CHK(hipMemcpy(A, stage.data(), arena, hipMemcpyHostToDevice));
    unsigned long long *O = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&O), 8 * out_words));
    CHK(hipMemset(O, 0, 8 * out_words));
    int wg0 = 0;
    std::vector<TimelineJob> jobs((size_t)njobs);
    for (int j = 0; j < njobs; j++) {
        // (columns: the group of a job is its trial, whose first row the offset table holds)
        jobs[(size_t)j] = TimelineJob{reinterpret_cast<const int4 *>(A + pl[(size_t)j].dst_a), reinterpret_cast<const int *>(A + pl[(size_t)j].dst_b), jr[j].nUE, census ? jr[j].group : j, wg0,
                                      jr[j].aT, jr[j].nslots, jr[j].E};
        wg0 += (jr[j].nUE + TL_TILE - 1) / TL_TILE;
    }
    TimelineJob *tj = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&tj), sizeof(TimelineJob) * jobs.size()));
    CHK(hipMemcpy(tj, jobs.data(), sizeof(TimelineJob) * jobs.size(), hipMemcpyHostToDevice));
    const size_t stride = (size_t)total_ue + GUARD, col_words = columns ? (size_t)sp.ncols * stride : 0;
    std::vector<int> cols(col_words, PATTERN);
    if (census) {
        CHK(launch_noma_census_kernel(tj, njobs, wgs, ax, scheme, XtabOut{O, O + cells}, nullptr));
    } else {
        int *D = nullptr;
        unsigned long long *T = nullptr;
        CHK(hipMalloc(reinterpret_cast<void **>(&D), 4 * col_words));
        CHK(hipMemcpy(D, cols.data(), 4 * col_words, hipMemcpyHostToDevice));
        CHK(hipMalloc(reinterpret_cast<void **>(&T), 8 * offset.size()));
        CHK(hipMemcpy(T, offset.data(), 8 * offset.size(), hipMemcpyHostToDevice));
        CHK(launch_noma_columns_kernel(tj, njobs, wgs, sp, ColumnsOut{D, (unsigned long long)stride, T, O}, nullptr));
        CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(cols.data(), D, 4 * col_words, hipMemcpyDeviceToHost));
    }
    CHK(hipDeviceSynchronize());

    std::vector<unsigned long long> res(4 + out_words);
    res[0] = (unsigned long long)MAGIC; res[1] = census ? 9ull : 10ull; res[2] = (unsigned long long)scheme; res[3] = (unsigned long long)wgs;
    CHK(hipMemcpy(res.data() + 4, O, 8 * out_words, hipMemcpyDeviceToHost));
    FILE *g = fopen(argv[2], "wb");
    if (!g) return fail("cannot open the result file");
    size_t put = fwrite(res.data(), 8, res.size(), g);
    if (columns) put += fwrite(cols.data(), 4, cols.size(), g);
    if (fclose(g) != 0 || put != res.size() + cols.size()) return fail("result file: short write");
    return 0;
}
