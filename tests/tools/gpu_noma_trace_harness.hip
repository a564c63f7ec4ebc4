// tests/tools/gpu_noma_trace_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::noma_trace_kernel launched directly, through launch_noma_trace_kernel, on rows
// of this program's own, filled from a case file that tests/tools/noma_trace_cases.py writes: (slot, sector) rows no trial writes.  The kernel's source file is
// compiled into this program as it is; no product entry point is involved.  The frame (arguments, case file, placement, upload, result file) is
// tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md and tests/tools/NOMA_TRACE.md.
//
// CASE header[8] = magic, kind 21, njobs, 0, bins, bin_ms, ngroups, 0; a job row is nrows, group, 1, accessTime, 0, 0, 0, 0 and its arrays are the frame's
//   form-1 pair: nrows filler words (never handed to the kernel), then rows[nrows][8] — tx, used, singles, granted, pairs, pair_one and two words the kernel
//   must not look at
// RESULT (int64) header[4] = magic, kind, scheme, workgroups; then the six series [ngroups][6][bins] and the scalars [ngroups][NT_SCALARS], each followed by
//   GUARD words at PATTERN (the outputs themselves are zeroed before the launch: the kernel adds to them)
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_trace.hip"

#define HARNESS_PROGRAM "gpu_noma_trace_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_noma_trace_harness CASE RESULT SCHEME | --check CASE | --constants";
constexpr int PATTERN = 0x7FFF7FFF, GUARD = 64;

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] { printf("NT_TILE %d\nNT_THREADS %d\nNT_WINDOW %d\nNT_SCALARS %d\n", NT_TILE, NT_THREADS, NT_WINDOW, NT_SCALARS); }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int scheme = a.check ? 0 : atoi(a.v[0]);
    if (scheme < 0 || scheme > 1) return fail("SCHEME is 0 or 1");

    Case c;
    if (const int e = c.read(a.in, 8, {21}, 1 << 12)) return e;
    const int bins = c.w[4], bin_ms = c.w[5], ngroups = c.w[6];
    if (bins < 1 || bins > PRACH_TRACE_MAX_BINS || bin_ms < 1 || ngroups < 1 || ngroups > 64 || c.w[3] || c.w[7]) return fail("case file: spec out of range");
    const Rule rule{false, ngroups, NT_TILE, E_UNUSED, 1ll << 22, false};
    for (int j = 0; j < c.njobs; j++)
        if (c.rows[j].form != 1 || c.rows[j].aT < 1 || c.rows[j].aT > 1000) return fail("job: form / accessTime out of range"); // (slot * accessTime stays far below 2^31)
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, zeroed outputs with patterned guards; ONE launch
    if (const int e = c.upload()) return e;
    NomaTraceJob *tj = nullptr;
    if (const int e = c.table(rule, tj, [](const JobRow &r, const unsigned char *, const unsigned char *b, int group, int wg0) {
            return NomaTraceJob{reinterpret_cast<const int4 *>(b), r.nUE, group, wg0, r.aT};
        })) return e;
    const size_t ser = (size_t)ngroups * 6 * (size_t)bins, sc = (size_t)ngroups * NT_SCALARS, total = 6 * (ser + GUARD) + sc + GUARD;
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * total, PATTERN)) return e;
    NomaTraceOut out{};
    for (int q = 0; q < 6; q++) { out.series[q] = O + (size_t)q * (ser + GUARD); CHK(hipMemset(out.series[q], 0, 8 * ser)); }
    out.scalars = O + 6 * (ser + GUARD);
    CHK(hipMemset(out.scalars, 0, 8 * sc));
    CHK(launch_noma_trace_kernel(tj, c.njobs, c.wgs, bins, bin_ms, scheme, out, nullptr));
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 21ull, (unsigned long long)scheme, (unsigned long long)c.wgs};
    return write_result(a.out, head, sizeof head, {{O, 8 * total}});
}
