// tests/tools/gpu_noma_select_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::noma_summary_kernel and prach::noma_pick_kernel launched directly, through
// their launch functions, on buffers of this program's own, filled from a case file that tests/tools/noma_select_cases.py writes: per-UE state no simulation
// leaves behind.  The kernels' source file is compiled into this program as it is; no product entry point is involved.  The frame (arguments, case file,
// placement, upload, result file) is tests/tools/harness_frame.h; the file formats are in tests/tools/HARNESS.md.
//
// CASE header[32] = magic, kind (11 summary, 12 pick), njobs, 0, spec (15 or 17 words); a row's group is the job's number, word 5 its E >= 0
//   spec, summary: who, nfields, field[4], nq, permille[8]      pick: who, nclauses, clause[4] = {field, lo, hi}, order, key_field, k
// RESULT (int64) header[4] = magic, kind, threads, njobs; everything behind it at PATTERN before the launch; pick: the int32 rows and GUARD words at the end
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_select.hip"

#define HARNESS_PROGRAM "gpu_noma_select_harness"
#include "harness_frame.h"

// prach_host.c's judgement of the two specs, restated for this program (it links no product object)
extern "C" int prach_internal_noma_summary_spec_ok(const prach_noma_summary_spec *s) {
    if (!s || s->who <= 0 || (s->who & ~15) != 0 || s->nfields < 1 || s->nfields > PRACH_NOMA_SUMMARY_MAX_FIELDS || s->nq < 1 || s->nq > PRACH_SUMMARY_MAX_Q || s->reserved[0] ||
        s->reserved[1]) return 0;
    for (int x = 0; x < PRACH_NOMA_SUMMARY_MAX_FIELDS; x++)
        if (x < s->nfields ? (s->field[x] < 0 || s->field[x] >= PRACH_NOMA_NFIELDS) : s->field[x] != 0) return 0;
    for (int l = 0; l < s->nq; l++)
        if (s->permille[l] < 1 || s->permille[l] > 1000) return 0;
    return 1;
}
extern "C" int prach_internal_noma_pick_spec_ok(const prach_pick_spec *s) {
    if (!s || s->who <= 0 || (s->who & ~15) != 0 || s->nclauses < 0 || s->nclauses > PRACH_PICK_MAX_CLAUSES || s->k < 1 || s->k > PRACH_PICK_MAX_K || s->reserved != 0 ||
        s->key_field < 0 || s->key_field >= PRACH_NOMA_NFIELDS) return 0;
    if (s->order != PRACH_PICK_BY_INDEX && s->order != PRACH_PICK_LARGEST && s->order != PRACH_PICK_SMALLEST) return 0;
    if (s->order == PRACH_PICK_BY_INDEX && s->key_field != PRACH_NOMA_ONE) return 0;
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++) {
        const prach_pick_clause *q = &s->clause[c];
        if (c < s->nclauses ? (q->field < 0 || q->field >= PRACH_NOMA_NFIELDS || q->lo < 0 || q->lo > q->hi) : (q->field || q->lo || q->hi)) return 0;
    }
    return 1;
}

static const char USAGE[] = "usage: gpu_noma_select_harness CASE RESULT THREADS | --check CASE | --constants";
constexpr int PATTERN = 0x7FFF7FFF, GUARD = 64;

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("NS_SCHED_CAP %d\nNS_COARSE %d\nNS_FINE %d\nNS_MAX_KEY %d\nNSM_WORDS %d\nPK_ROW_WORDS %d\nPK_SCALARS %d\nNSM_LDS_WORDS %d\nNS_LDS_WORDS %d\n", noma_select_sched_cap(),
               NS_COARSE, NS_FINE, NS_MAX_KEY, NSM_WORDS, PK_ROW_WORDS, PK_SCALARS, NSM_FIXED_WORDS, NS_FIXED_WORDS);
    }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int threads = a.check ? 512 : atoi(a.v[0]);
    if (threads != 512 && threads != 1024) return fail("THREADS is 512 or 1024");

    Case c;
    if (const int e = c.read(a.in, 32, {11, 12}, 1 << 12)) return e;
    const std::vector<int> &w = c.w;
    const bool summary = w[1] == 11;
    const int njobs = c.njobs;
    prach_noma_summary_spec ss{};
    prach_pick_spec ps{};
    if (summary) {
        ss.who = w[4]; ss.nfields = w[5]; ss.nq = w[10];
        for (int x = 0; x < 4; x++) ss.field[x] = w[6 + x];
        for (int l = 0; l < 8; l++) ss.permille[l] = w[11 + l];
        if (!prach_internal_noma_summary_spec_ok(&ss)) return fail("case file: summary spec out of range");
    } else {
        ps.who = w[4]; ps.nclauses = w[5]; ps.order = w[18]; ps.key_field = w[19]; ps.k = w[20];
        for (int q = 0; q < 4; q++) ps.clause[q] = prach_pick_clause{w[6 + 3 * q], w[7 + 3 * q], w[8 + 3 * q]};
        if (!prach_internal_noma_pick_spec_ok(&ps)) return fail("case file: pick spec out of range");
    }
    const Rule rule{true, 0, 0, E_NOT_NEGATIVE, 1ll << 24, false}; // (a job's group is its number: the offset of its stores)
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, patterned outputs; ONE launch
    if (const int e = c.upload()) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    const int scap = c.max_slots < noma_select_sched_cap() ? c.max_slots : noma_select_sched_cap(); // the engine's rule
    // 64-bit words: the summary's rows, or the pick's scalars; then, pick only, the rows and the guard as 32-bit words
    const size_t head_words = summary ? (size_t)njobs * NSM_WORDS : (size_t)njobs * PK_SCALARS;
    const size_t row_ints = summary ? 0 : (size_t)njobs * (size_t)ps.k * 2 * PK_ROW_WORDS + GUARD;
    unsigned long long *H = nullptr;
    int *R = nullptr;
    if (const int e = device_words(H, 2 * head_words, PATTERN)) return e;
    if (const int e = device_words(R, row_ints, PATTERN)) return e;
    if (summary) CHK(launch_noma_summary_kernel(tj, njobs, ss, threads, scap, H, nullptr));
    else CHK(launch_noma_pick_kernel(tj, njobs, ps, threads, scap, reinterpret_cast<unsigned long long *>(R), H, nullptr));
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, summary ? 11ull : 12ull, (unsigned long long)threads, (unsigned long long)njobs};
    return write_result(a.out, head, sizeof head, {{H, 8 * head_words}, {R, 4 * row_ints}});
}
