// tests/tools/gpu_noma_gain_harness.hip — TEST INFRASTRUCTURE (GPU box): the two kernels of prach_noma_gain.hip launched directly, through their launch
// functions, on buffers of this program's own, filled from a case file and a side file that tests/tools/noma_gain_cases.py writes: per-UE records, ln(gain)
// values and levels no simulation leaves behind.  The kernels' source file is compiled into this program as it is; no product entry point is involved.  The
// frame (arguments, case file, placement, upload, result file) is tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md and NOMA_GAIN.md.
//
// CASE header[16] = magic, 14, njobs, bins, width, lo, ngroups; word 5 of a row is E >= 0
// SIDE  float64 lgain[total UEs] in job order, then int32 level[total UEs] in job order
// MODE 0 / 1: the reducer under that scheme on the side file's LEVELS.
//   RESULT (uint64) header[4] = magic, 14, mode, workgroups; then the six series [ngroups][6][bins] each and scalars[ngroups][NG_SCALARS], all zero before the launch
// MODE 2: the level pre-pass on the side file's LGAIN with a list of EDGE_CAP entries (0 .. NG_EDGE_CAP).
//   RESULT header[4] as above, then as uint32: the list's two header words, 2 x EDGE_CAP entry words and GUARD words behind them (the list zeroed, the guard
//   words at PATTERN before the launch), then the level column of every job in job order (at PATTERN before the launch)
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_gain.hip"

#define HARNESS_PROGRAM "gpu_noma_gain_harness"
#include "harness_frame.h"

static const char USAGE[] = "usage: gpu_noma_gain_harness CASE RESULT MODE SIDE [EDGE_CAP] | --check CASE | --constants";
static constexpr int GUARD = 64, PATTERN = 0x7FFF7FFF;

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("TL_TILE %d\nTL_THREADS %d\nTILE_SCHED_CAP %d\nNG_SCALARS %d\nNG_EDGE_CAP %d\nNG_LDS_MAX_BINS %d\nNG_MAX_ADDEND %d\nNG_LEVEL_BAND %.17g\nNG_LEVEL_RANGE %.17g\n", TL_TILE,
               TL_THREADS, TILE_SCHED_CAP, NG_SCALARS, NG_EDGE_CAP, NG_LDS_MAX_BINS, NG_MAX_ADDEND, NG_LEVEL_BAND, NG_LEVEL_RANGE);
    }, a);
    if (rc >= 0) return rc;
    if (a.check ? a.n != 0 : (a.n != 2 && a.n != 3)) return fail(USAGE);
    const int mode = a.check ? 0 : atoi(a.v[0]);
    const int edge_cap = a.n == 3 ? atoi(a.v[2]) : NG_EDGE_CAP;

    Case c;
    if (const int e = c.read(a.in, 16, {14}, 1 << 16)) return e;
    const std::vector<int> &w = c.w;
    const int njobs = c.njobs, bins = w[3], width = w[4], lo = w[5], ngroups = w[6];
    if (bins < 1 || bins > PRACH_NOMA_GAIN_MAX_BINS || width < 1 || ngroups < 1 || ngroups > 64) return fail("case file: bins / width / ngroups out of range");
    if (mode < 0 || mode > 2) return fail("mode out of range");
    if (edge_cap < 0 || edge_cap > NG_EDGE_CAP) return fail("edge capacity out of range");
    const size_t part = (size_t)ngroups * 6 * (size_t)bins, out_words = 6 * part + (size_t)ngroups * NG_SCALARS;
    if (out_words > (size_t)1 << 26) return fail("case file: outputs too large");
    const Rule rule{true, ngroups, TL_TILE, E_NOT_NEGATIVE, 1ll << 24, false};
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- the side file: one ln(gain) and one level per UE of the case
    const size_t total = (size_t)c.total_ue;
    std::vector<double> lgain(total);
    std::vector<int> level(total);
    {
        FILE *f = fopen(a.v[1], "rb");
        if (!f) return fail("cannot open the side file");
        const bool ok = fread(lgain.data(), 8, total, f) == total && fread(level.data(), 4, total, f) == total && fgetc(f) == EOF;
        fclose(f);
        if (!ok) return fail("side file: not one float64 and one int32 per UE");
    }

    // ---- device: arena, the two columns, job table, outputs; ONE launch
    if (const int e = c.upload()) return e;
    double *dlg = nullptr;
    int *dlv = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&dlg), 8 * total));
    CHK(hipMemcpy(dlg, lgain.data(), 8 * total, hipMemcpyHostToDevice));
    if (mode == 2) { if (const int e = device_words(dlv, total, PATTERN)) return e; }
    else {
        CHK(hipMalloc(reinterpret_cast<void **>(&dlv), 4 * total));
        CHK(hipMemcpy(dlv, level.data(), 4 * total, hipMemcpyHostToDevice));
    }
    NomaGainJob *gj = nullptr;
    size_t at = 0; // the job's first UE in the two columns
    if (const int e = c.table(rule, gj, [&](const JobRow &r, const unsigned char *logs, const unsigned char *sched, int group, int wg0) {
            NomaGainJob j;
            static_cast<TimelineJob &>(j) = TimelineJob{reinterpret_cast<const int4 *>(logs), reinterpret_cast<const int *>(sched), r.nUE, group, wg0, r.aT, r.nslots, r.E};
            j.lgain = dlg + at; j.level = dlv + at;
            at += (size_t)r.nUE;
            return j;
        })) return e;
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 14ull, (unsigned long long)mode, (unsigned long long)c.wgs};
    if (mode == 2) {
        const size_t list_words = 2 + 2 * (size_t)edge_cap;
        unsigned *E = nullptr;
        if (const int e = device_words(E, list_words + GUARD, PATTERN)) return e;
        CHK(hipMemset(E, 0, 4 * list_words));
        CHK(launch_noma_gain_levels(gj, njobs, c.wgs, E, edge_cap, nullptr));
        CHK(hipDeviceSynchronize());
        return write_result(a.out, head, sizeof head, {{E, 4 * (list_words + GUARD)}, {dlv, 4 * total}});
    }
    unsigned long long *O = nullptr;
    if (const int e = device_words(O, 2 * out_words, 0)) return e;
    CHK(launch_noma_gain_kernel(gj, njobs, c.wgs, bins, width, lo, mode, NomaGainOut{{O, O + part, O + 2 * part, O + 3 * part, O + 4 * part, O + 5 * part}, O + 6 * part}, nullptr));
    CHK(hipDeviceSynchronize());
    return write_result(a.out, head, sizeof head, {{O, 8 * out_words}});
}
