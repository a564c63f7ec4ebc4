// tests/tools/gpu_pick_harness.hip — TEST INFRASTRUCTURE (GPU box): prach::pick_kernel launched directly, through launch_pick_kernel, on buffers of this
// program's own, filled from a case file that tests/tools/pick_cases.py writes: per-UE state no simulation leaves behind.  The kernel's source file is
// compiled into this program as it is; no product entry point is involved (the spec check of prach_host.c is restated below: the host C file is not part
// of this program).  The frame (arguments, case file, placement, upload, result file) is tests/tools/harness_frame.h; the file formats are in
// tests/tools/HARNESS.md.
//
// CASE header[32] = magic, 4, njobs, who, nclauses, clause[4][3] = field, lo, hi, order, key_field, k; a row's group is its trial, word 5 its E
// RESULT (uint64) header[4] = magic, 4, threads, njobs
#include "../../5g-nr-randomaccess_amd/csrc/prach_pick.hip"

#define HARNESS_PROGRAM "gpu_pick_harness"
#include "harness_frame.h"

extern "C" int prach_internal_pick_spec_ok(const prach_pick_spec *s) { // prach_host.c's, for this program
    if (!s || s->who <= 0 || (s->who & ~7) != 0 || s->nclauses < 0 || s->nclauses > PRACH_PICK_MAX_CLAUSES || s->k < 1 || s->k > PRACH_PICK_MAX_K || s->reserved != 0 ||
        s->key_field < 0 || s->key_field >= PRACH_XTAB_NFIELDS || s->order < 0 || s->order > 2 || (s->order == PRACH_PICK_BY_INDEX && s->key_field != 0)) return 0;
    for (int c = 0; c < PRACH_PICK_MAX_CLAUSES; c++) {
        const prach_pick_clause *q = &s->clause[c];
        if (c < s->nclauses ? (q->field < 0 || q->field >= PRACH_XTAB_NFIELDS || q->lo < 0 || q->lo > q->hi) : (q->field || q->lo || q->hi)) return 0;
    }
    return 1;
}

static const char USAGE[] = "usage: gpu_pick_harness CASE RESULT THREADS | --check CASE | --constants";

int main(int argc, char **argv) {
    using namespace prach;
    Args a;
    const int rc = arguments(argc, argv, USAGE, [] {
        printf("PK_ROW_WORDS %d\nPK_SCALARS %d\nPK_MAX_KEY %d\nPK_SCHED_CAP %d\nPK_COARSE %d\nPK_FINE %d\nPRACH_PICK_MAX_K %d\nPRACH_PICK_MAX_CLAUSES %d\nTL_MAX_SOJOURN %d\n", PK_ROW_WORDS,
               PK_SCALARS, PK_MAX_KEY, PK_SCHED_CAP, PK_COARSE, PK_FINE, PRACH_PICK_MAX_K, PRACH_PICK_MAX_CLAUSES, TL_MAX_SOJOURN);
    }, a);
    if (rc >= 0) return rc;
    if (a.n != (a.check ? 0 : 1)) return fail(USAGE);
    const int threads = a.check ? 512 : atoi(a.v[0]);
    if (threads != 512 && threads != 1024) return fail("threads: 512 or 1024");

    Case c;
    if (const int e = c.read(a.in, 32, {4}, 1 << 12)) return e;
    const std::vector<int> &w = c.w;
    prach_pick_spec sp{};
    sp.who = w[3]; sp.nclauses = w[4];
    for (int q = 0; q < PRACH_PICK_MAX_CLAUSES; q++) sp.clause[q] = prach_pick_clause{w[5 + 3 * q], w[6 + 3 * q], w[7 + 3 * q]};
    sp.order = w[17]; sp.key_field = w[18]; sp.k = w[19];
    if (!prach_internal_pick_spec_ok(&sp)) return fail("case file: a bad spec"); // (k bounds every row store)
    const Rule rule{true, c.njobs, 0, E_PASSED, 1ll << 24, false};             // (a trial index is the offset of the stores)
    if (const int e = c.place(rule)) return e;
    if (a.check) return 0;

    // ---- device: arena, job table, outputs filled with a pattern (what the kernel does not write stays at it: the rows behind `stored`, and everything
    // of a trial no job names); ONE launch
    if (const int e = c.upload()) return e;
    const size_t sc_words = (size_t)c.njobs * PK_SCALARS, row_words = (size_t)c.njobs * (size_t)sp.k * PK_ROW_WORDS;
    unsigned long long *O = nullptr; // scalars, then rows (the rows start at a multiple of 64 bytes)
    if (const int e = device_words(O, 2 * (sc_words + row_words), 0x5A5A5A5A)) return e;
    TimelineJob *tj = nullptr;
    if (const int e = c.timeline_table(rule, tj)) return e;
    CHK(launch_pick_kernel(tj, c.njobs, sp, threads, c.max_slots < PK_SCHED_CAP ? c.max_slots : PK_SCHED_CAP, O + sc_words, O, nullptr)); // (the engine's staging rule)
    CHK(hipDeviceSynchronize());
    const unsigned long long head[4] = {(unsigned long long)MAGIC, 4ull, (unsigned long long)threads, (unsigned long long)c.njobs};
    return write_result(a.out, head, sizeof head, {{O, 8 * (sc_words + row_words)}});
}
