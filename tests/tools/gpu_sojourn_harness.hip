// tests/tools/gpu_sojourn_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::sojourn_kernel launched directly, through launch_sojourn_kernel, on buffers
// of this program's own, filled from a case file that tests/tools/sojourn_cases.py writes: per-UE state no simulation leaves behind.  The kernel's source
// file is compiled into this program as it is; no product entry point is involved.  The frame (arguments, case file, placement, upload, result file) is
// tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// CASE header[16] = magic, 2, njobs, rows, row_ms, delay_bins, delay_bin_ms, ngroups     RESULT (uint64) header[4] = magic, 2, scheme, workgroups
#include "../../5g-nr-randomaccess_amd/csrc/prach_sojourn.hip"

#define HARNESS_PROGRAM "gpu_sojourn_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_sojourn_harness CASE RESULT SCHEME | --check CASE | --constants";

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("TL_TILE %d\nTL_THREADS %d\nTL_MAX_SOJOURN %d\nSJ_WINDOW_WORDS %d\nSJ_SCHED_CAP %d\nSJ_SCALARS %d\n", TL_TILE, TL_THREADS, TL_MAX_SOJOURN, SJ_WINDOW_WORDS,
               SJ_SCHED_CAP, SJ_SCALARS);
    }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int scheme = a.check ? 0 : atoi(a.v[0]);

    Case c;
    if (const int e = c.read(a.in, 16, {2}, 1 << 16)) return e;
    const int rows = c.w[3], row_ms = c.w[4], dbins = c.w[5], dwidth = c.w[6], ngroups = c.w[7];
    if (ngroups < 1 || ngroups > 64 || row_ms < 1 || dwidth < 1) return fail("case file: ngroups / widths out of range");
    if (rows < 1 || rows > PRACH_SOJOURN_MAX_ARRIVAL_BINS || dbins < 1 || dbins > PRACH_SOJOURN_MAX_DELAY_BINS) return fail("case file: bin counts out of range");
    if (scheme < 0 || scheme > 1) return fail("scheme out of range");
    const size_t ng = (size_t)ngroups, cells = ng * (size_t)rows * (size_t)dbins, per_row = ng * (size_t)rows;
    const size_t out_words = cells + 2 * per_row + ng * SJ_SCALARS;
    if (out_words > (size_t)1 << 26) return fail("case file: outputs too large");
    const Rule rule{true, ngroups, TL_TILE, E_UNUSED, 1ll << 24, false};
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, zeroed outputs; ONE launch
    if (const int e = c.upload()) return e;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0)) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    CHK(launch_sojourn_kernel(tj, c.njobs, c.wgs, rows, row_ms, dbins, dwidth, scheme, SojournOut{O, O + cells, O + cells + per_row, O + cells + 2 * per_row}, nullptr));
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 2ull, (unsigned long long)scheme, (unsigned long long)c.wgs};
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}});
}
