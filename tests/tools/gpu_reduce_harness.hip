// tests/tools/gpu_reduce_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::dist_kernel and prach::timeline_kernel launched directly, through
// launch_dist_kernel / launch_timeline_kernel, on buffers of this program's own, filled from a case file that tests/tools/reduce_cases.py writes: per-UE
// state no simulation leaves behind.  The kernels' source files are compiled into this program as they are; no product entry point is involved.  The frame
// (arguments, case file, placement, upload, result file) is tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// usage: gpu_reduce_harness CASE RESULT SCHEME | --check CASE | --constants
// CASE header[16] = magic, kind (0 dist, 1 timeline), njobs, bins, width, ngroups     RESULT (uint64) header[4] = magic, kind, scheme, workgroups
#include "../../5g-nr-randomaccess_amd/csrc/prach_dist.hip"
#include "../../5g-nr-randomaccess_amd/csrc/prach_timeline.hip"

#define HARNESS_PROGRAM "gpu_reduce_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_reduce_harness CASE RESULT SCHEME | --check CASE | --constants";

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("DIST_TILE %d\nDIST_THREADS %d\nDIST_PTC_BINS %d\nDIST_SCALARS %d\nTL_TILE %d\nTL_THREADS %d\nTL_WINDOW %d\nTL_MAX_SOJOURN %d\nTL_SCHED_CAP %d\nTL_SCALARS %d\n",
               DIST_TILE, DIST_THREADS, PB, DIST_SCALARS, TL_TILE, TL_THREADS, TL_WINDOW, TL_MAX_SOJOURN, TL_SCHED_CAP, TL_SCALARS);
    }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int scheme = a.check ? 0 : atoi(a.v[0]);

    Case c;
    if (const int e = c.read(a.in, 16, {0, 1}, 1 << 16)) return e;
    const int kind = c.w[1], bins = c.w[3], width = c.w[4], ngroups = c.w[5];
    if (ngroups < 1 || ngroups > 4096 || width < 1) return fail("case file: ngroups / width out of range");
    if (bins < 1 || bins > (kind == 0 ? PRACH_DIST_MAX_DELAY_BINS : PRACH_TIMELINE_MAX_BINS)) return fail("case file: bins out of range");
    if (scheme < 0 || scheme > (kind == 0 ? 2 : 1)) return fail("scheme out of range");
    const Rule rule{kind == 1, ngroups, kind == 0 ? DIST_TILE : TL_TILE, E_UNUSED, 1ll << 24, false};
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, zeroed outputs; ONE launch
    if (const int e = c.upload()) return e;
    const size_t ng = (size_t)ngroups, per_series = ng * (size_t)bins;
    const size_t out_words = kind == 0 ? per_series + ng * PB + ng * DIST_SCALARS : 5 * per_series + ng * TL_SCALARS;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0)) return e;
    if (kind == 0) {
        DistJob *dj = nullptr;
        const int e = c.table(rule, dj, [](const JobRow &r, const unsigned char *t, const unsigned char *p, int group, int wg0) {
            return DistJob{reinterpret_cast<const int *>(t), reinterpret_cast<const int *>(p), r.nUE, group, wg0, r.form};
        });
        if (e) return e;
        CHK(launch_dist_kernel(dj, c.njobs, c.wgs, bins, width, scheme, O, O + per_series, O + per_series + ng * PB, nullptr));
    } else {
        TimelineJob *tj = nullptr;
        if (const int e = c.timeline_table(rule, tj)) return e;
        const TimelineOut out{O, O + per_series, O + 2 * per_series, O + 3 * per_series, O + 4 * per_series, O + 5 * per_series};
        CHK(launch_timeline_kernel(tj, c.njobs, c.wgs, bins, width, scheme, out, nullptr));
    }
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, (unsigned long long)kind, (unsigned long long)scheme, (unsigned long long)c.wgs};
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}});
}
