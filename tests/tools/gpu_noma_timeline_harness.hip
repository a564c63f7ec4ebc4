// tests/tools/gpu_noma_timeline_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::noma_timeline_kernel launched directly, through its launch function, on
// buffers of this program's own, filled from a case file that tests/tools/noma_timeline_cases.py writes: per-UE state no simulation leaves behind.  The
// kernel's source file is compiled into this program as it is; no product entry point is involved.  The frame (arguments, case file, placement, upload,
// result file) is tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// CASE header[16] = magic, 13, njobs, bins, bin_ms, ngroups, window (0: NTL_WINDOW); word 5 of a row is E >= 0
// RESULT (uint64) header[4] = magic, 13, scheme, workgroups; then the six series [ngroups][6][bins] each and scalars[ngroups][NTL_SCALARS], all zero before the
// launch
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_timeline.hip"

#define HARNESS_PROGRAM "gpu_noma_timeline_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_noma_timeline_harness CASE RESULT SCHEME | --check CASE | --constants";

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("TL_TILE %d\nTL_THREADS %d\nNTL_WINDOW %d\nNTL_WINDOW_MAX %d\nNTL_MAX_SOJOURN %d\nTILE_SCHED_CAP %d\nNTL_SCALARS %d\n", TL_TILE, TL_THREADS, NTL_WINDOW, NTL_WINDOW_MAX,
               NTL_MAX_SOJOURN, TILE_SCHED_CAP, NTL_SCALARS);
    }, a);
    if (rc >= 0) return rc;
    if (a.check ? a.n != 0 : a.n != 1) return fail(USAGE);
    const int scheme = a.n == 1 ? atoi(a.v[0]) : 0;

    Case c;
    if (const int e = c.read(a.in, 16, {13}, 1 << 16)) return e;
    const std::vector<int> &w = c.w;
    const int njobs = c.njobs, bins = w[3], bin_ms = w[4], ngroups = w[5], window = w[6] ? w[6] : NTL_WINDOW;
    if (bins < 1 || bins > PRACH_TIMELINE_MAX_BINS || bin_ms < 1 || ngroups < 1 || ngroups > 64) return fail("case file: bins / bin_ms / ngroups out of range");
    if (window < 1 || window > NTL_WINDOW_MAX) return fail("case file: window out of range");
    if (scheme < 0 || scheme > 1) return fail("scheme out of range");
    const size_t part = (size_t)ngroups * 6 * (size_t)bins, out_words = 6 * part + (size_t)ngroups * NTL_SCALARS;
    if (out_words > (size_t)1 << 26) return fail("case file: outputs too large");
    const Rule rule{true, ngroups, TL_TILE, E_NOT_NEGATIVE, 1ll << 24, false};
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, zeroed counters; ONE launch
    if (const int e = c.upload()) return e;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0)) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    CHK(launch_noma_timeline_kernel(tj, njobs, c.wgs, bins, bin_ms, scheme, window,
                                    NomaTimelineOut{{O, O + part, O + 2 * part, O + 3 * part, O + 4 * part, O + 5 * part}, O + 6 * part}, nullptr));
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 13ull, (unsigned long long)scheme, (unsigned long long)c.wgs};
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}});
}
