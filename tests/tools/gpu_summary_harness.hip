// tests/tools/gpu_summary_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::summary_kernel launched directly, through launch_summary_kernel, on buffers
// of this program's own, filled from a case file that tests/tools/summary_cases.py writes: per-UE state no simulation leaves behind.  The kernel's source
// file is compiled into this program as it is; no product entry point is involved.  The frame (arguments, case file, placement, upload, result file) is
// tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// CASE header[16] = magic, 3, njobs, nq, permille[8]; a row's group is the row of its store     RESULT (uint64) header[4] = magic, 3, threads, njobs
#include "../../5g-nr-randomaccess_amd/csrc/prach_summary.hip"

#define HARNESS_PROGRAM "gpu_summary_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_summary_harness CASE RESULT THREADS | --check CASE | --constants";

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("SM_WORDS %d\nSM_MAX_VALUE %d\nSM_SCHED_CAP %d\nSM_COARSE %d\nSM_FINE %d\nPRACH_SUMMARY_MAX_Q %d\nTL_MAX_SOJOURN %d\n", SM_WORDS, SM_MAX_VALUE, SM_SCHED_CAP,
               SM_COARSE, SM_FINE, PRACH_SUMMARY_MAX_Q, TL_MAX_SOJOURN);
    }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int threads = a.check ? 512 : atoi(a.v[0]);
    if (threads != 512 && threads != 1024) return fail("threads: 512 or 1024");

    Case c;
    if (const int e = c.read(a.in, 16, {3}, 1 << 16)) return e;
    SummaryLevels lv{};
    lv.nq = c.w[3];
    if (lv.nq < 1 || lv.nq > PRACH_SUMMARY_MAX_Q) return fail("case file: nq out of range");
    for (int l = 0; l < lv.nq; l++) {
        lv.permille[l] = c.w[4 + l];
        if (lv.permille[l] < 1 || lv.permille[l] > 1000) return fail("case file: level out of range");
    }
    const Rule rule{true, c.njobs, 0, E_UNUSED, 1ll << 24, false}; // (a row index is the offset of a store)
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, outputs filled with a pattern (the kernel stores whole rows; a row no job names stays at it and fails the comparison)
    if (const int e = c.upload()) return e;
    const size_t out_words = (size_t)c.njobs * SM_WORDS;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0x5A5A5A5A)) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    CHK(launch_summary_kernel(tj, c.njobs, lv, threads, c.max_slots < SM_SCHED_CAP ? c.max_slots : SM_SCHED_CAP, O, nullptr)); // (the engine's staging rule)
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 3ull, (unsigned long long)threads, (unsigned long long)c.njobs};
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}});
}
