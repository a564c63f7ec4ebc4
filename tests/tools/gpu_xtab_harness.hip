// tests/tools/gpu_xtab_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::xtab_kernel launched directly, through launch_xtab_kernel, on buffers of this
// program's own, filled from a case file that tests/tools/xtab_cases.py writes: per-UE state no simulation leaves behind.  The kernel's source file is
// compiled into this program as it is; no product entry point is involved.  The frame (arguments, case file, placement, upload, result file) is
// tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// CASE header[16] = magic, 3, njobs, who, row_field, row_width, row_bins, col_field, col_width, col_bins, ngroups; word 5 of a row is E >= 0
// RESULT (uint64) header[4] = magic, 3, scheme, workgroups
#include "../../5g-nr-randomaccess_amd/csrc/prach_xtab.hip"

#define HARNESS_PROGRAM "gpu_xtab_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_xtab_harness CASE RESULT SCHEME | --check CASE | --constants";

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("TL_TILE %d\nTL_THREADS %d\nXT_WINDOW_WORDS %d\nXT_COPY_WORDS %d\nXT_SCHED_CAP %d\nXT_SCALARS %d\n", TL_TILE, TL_THREADS, XT_WINDOW_WORDS, XT_COPY_WORDS,
               XT_SCHED_CAP, XT_SCALARS);
    }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int scheme = a.check ? 0 : atoi(a.v[0]);

    Case c;
    if (const int e = c.read(a.in, 16, {3}, 1 << 16)) return e;
    const std::vector<int> &w = c.w;
    const int ngroups = w[10];
    const XtabAxes ax{w[3], w[4], w[5], w[6], w[7], w[8], w[9]};
    if (ngroups < 1 || ngroups > 64 || ax.row_width < 1 || ax.col_width < 1) return fail("case file: ngroups / widths out of range");
    if (ax.row_bins < 1 || ax.row_bins > PRACH_XTAB_MAX_BINS || ax.col_bins < 1 || ax.col_bins > PRACH_XTAB_MAX_BINS) return fail("case file: bin counts out of range");
    if (ax.who < 1 || ax.who > 7 || ax.row_field < 0 || ax.row_field >= PRACH_XTAB_NFIELDS || ax.col_field < 0 || ax.col_field >= PRACH_XTAB_NFIELDS) return fail("case file: who / fields out of range");
    if (scheme < 0 || scheme > 1) return fail("scheme out of range");
    const size_t ng = (size_t)ngroups, cells = ng * ((size_t)ax.row_bins + 1) * ((size_t)ax.col_bins + 1);
    const size_t out_words = cells + ng * XT_SCALARS;
    if (out_words > (size_t)1 << 26) return fail("case file: outputs too large");
    const Rule rule{true, ngroups, TL_TILE, E_NOT_NEGATIVE, 1ll << 24, false};
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, zeroed outputs; ONE launch
    if (const int e = c.upload()) return e;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0)) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    CHK(launch_xtab_kernel(tj, c.njobs, c.wgs, ax, scheme, XtabOut{O, O + cells}, nullptr));
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 3ull, (unsigned long long)scheme, (unsigned long long)c.wgs};
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}});
}
