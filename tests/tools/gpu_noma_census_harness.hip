// tests/tools/gpu_noma_census_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::noma_census_kernel and prach::noma_columns_kernel launched directly,
// through their launch functions, on buffers of this program's own, filled from a case file that tests/tools/noma_census_cases.py writes: per-UE state no
// simulation leaves behind.  The kernels' source file is compiled into this program as it is; no product entry point is involved.  The frame (arguments,
// case file, placement, upload, result file) is tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// CASE header[32] = magic, 9, njobs, who, row_field, row_width, row_bins, col_field, col_width, col_bins, ngroups, ncols, field[16]; word 5 of a row is E >= 0
// RESULT (uint64) header[4] = magic, 9 (census) or 10 (columns), scheme, workgroups; columns: the int32 columns behind the scalars, GUARD words behind the
// rows of each, all at PATTERN before the launch
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_census.hip"

#define HARNESS_PROGRAM "gpu_noma_census_harness"
#include "harness_frame.h"

// prach_host.c's judgement of a columns spec, restated for this program (it links no product object)
extern "C" int prach_internal_noma_columns_spec_ok(const prach_columns_spec *s) {
    if (!s || s->ncols < 1 || s->ncols > PRACH_COL_MAX || s->reserved[0] || s->reserved[1] || s->reserved[2]) return 0;
    for (int c = 0; c < s->ncols; c++) {
        const int f = s->field[c];
        if (!((f >= 0 && f < PRACH_NOMA_NFIELDS) || (f >= PRACH_COL_RAW && f < PRACH_COL_RAW + 16))) return 0;
    }
    return 1;
}

static const char USAGE[] = "usage: gpu_noma_census_harness CASE RESULT census SCHEME | CASE RESULT columns | --check CASE [columns] | --constants";
constexpr int PATTERN = 0x7FFF7FFF, GUARD = 64;

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("TL_TILE %d\nTL_THREADS %d\nXT_WINDOW_WORDS %d\nNC_COPY_WORDS %d\nTILE_SCHED_CAP %d\nNC_SCALARS %d\nNCL_SCALARS %d\n", TL_TILE, TL_THREADS, XT_WINDOW_WORDS,
               noma_census_copy_words(), TILE_SCHED_CAP, NC_SCALARS, NCL_SCALARS);
    }, a);
    if (rc >= 0) return rc;
    const bool columns = a.n == 1 && !strcmp(a.v[0], "columns"), census = a.check ? a.n == 0 : a.n == 2 && !strcmp(a.v[0], "census");
    if (!census && !columns) return fail(USAGE);
    const int scheme = a.n == 2 ? atoi(a.v[1]) : 0;

    Case c;
    if (const int e = c.read(a.in, 32, {9}, 1 << 16)) return e;
    const std::vector<int> &w = c.w;
    const int njobs = c.njobs, ngroups = w[10];
    const XtabAxes ax{w[3], w[4], w[5], w[6], w[7], w[8], w[9]};
    prach_columns_spec sp{};
    sp.ncols = w[11];
    for (int q = 0; q < PRACH_COL_MAX; q++) sp.field[q] = w[12 + q];
    if (ngroups < 1 || ngroups > 64 || ax.row_width < 1 || ax.col_width < 1) return fail("case file: ngroups / widths out of range");
    if (ax.row_bins < 1 || ax.row_bins > PRACH_XTAB_MAX_BINS || ax.col_bins < 1 || ax.col_bins > PRACH_XTAB_MAX_BINS) return fail("case file: bin counts out of range");
    if (ax.who < 1 || ax.who > 15 || ax.row_field < 0 || ax.row_field >= PRACH_NOMA_NFIELDS || ax.col_field < 0 || ax.col_field >= PRACH_NOMA_NFIELDS) return fail("case file: who / fields out of range");
    if (columns && !prach_internal_noma_columns_spec_ok(&sp)) return fail("case file: columns out of range");
    if (scheme < 0 || scheme > 1) return fail("scheme out of range");
    const size_t ng = (size_t)ngroups, cells = ng * ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const size_t out_words = census ? cells + ng * NC_SCALARS : (size_t)njobs * NCL_SCALARS;
    if (out_words > (size_t)1 << 26) return fail("case file: outputs too large");
    const Rule rule{true, ngroups, TL_TILE, E_NOT_NEGATIVE, 1ll << 24, columns}; // (columns: the group of a job is its trial, whose first row the offset table holds)
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, zeroed counters, patterned columns; ONE launch
    if (const int e = c.upload()) return e;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0)) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    const size_t stride = (size_t)c.total_ue + GUARD, col_words = columns ? (size_t)sp.ncols * stride : 0;
    int *D = nullptr;
    if (census) {
        CHK(launch_noma_census_kernel(tj, njobs, c.wgs, ax, scheme, XtabOut{O, O + cells}, nullptr));
    } else {
        std::vector<unsigned long long> offset((size_t)njobs, 0); // a trial's first row: the UEs of the jobs before it
        for (int j = 1; j < njobs; j++) offset[(size_t)j] = offset[(size_t)j - 1] + (unsigned long long)c.rows[j - 1].nUE;
        unsigned long long *T = nullptr;
        if (const int e = device_words(D, col_words, PATTERN)) return e;
        CHK(hipMalloc(reinterpret_cast<void **>(&T), 8 * offset.size()));
        CHK(hipMemcpy(T, offset.data(), 8 * offset.size(), hipMemcpyHostToDevice));
        CHK(launch_noma_columns_kernel(tj, njobs, c.wgs, sp, ColumnsOut{D, (unsigned long long)stride, T, O}, nullptr));
    }
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, census ? 9ull : 10ull, (unsigned long long)scheme, (unsigned long long)c.wgs};
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}, {D, 4 * col_words}});
}
