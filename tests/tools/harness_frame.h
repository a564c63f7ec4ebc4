// tests/tools/harness_frame.h — TEST INFRASTRUCTURE: what the off-trial kernel harnesses (tests/tools/gpu_*_harness.hip) have in common, once.  A harness
// is a stand-alone program around ONE kernel source: it includes that source, defines HARNESS_PROGRAM (its name, for the messages), includes this header
// and keeps only what is its own — its spec words, its output layout and fill pattern, its launch call and its constants line.  tests/tools/HARNESS.md
// has the file formats.  Exit codes: 0 done, 2 a HIP error, 3 a bad file or argument (message on stderr).
//
//   PROGRAM CASE RESULT [ARG ...]    one launch: read the case, place the arrays, fill the outputs, launch, synchronise, write the result
//   PROGRAM --check CASE [ARG ...]   everything up to and including placement; no HIP call; exit code 0 or 3
//   PROGRAM --constants              the kernel's compile-time constants, one "NAME value" per line; no HIP call
#pragma once
#ifndef HARNESS_PROGRAM
#error "define HARNESS_PROGRAM (the program's name) before including harness_frame.h"
#endif

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#define CHK(call)                                                                                                 \
    do {                                                                                                          \
        const hipError_t rc_ = (call);                                                                            \
        if (rc_ != hipSuccess) {                                                                                  \
            fprintf(stderr, HARNESS_PROGRAM ": %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__);     \
            return 2;                                                                                             \
        }                                                                                                         \
    } while (0)

namespace {

constexpr int MAGIC = 0x52445543;

int fail(const char *what) {
    fprintf(stderr, HARNESS_PROGRAM ": %s\n", what);
    return 3;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- the command line: `a.v[0 .. a.n)` are the program's own arguments behind CASE RESULT (or behind --check CASE)
struct Args { bool check = false; const char *in = nullptr, *out = nullptr; int n = 0; char **v = nullptr; };

// -1: go on with `a`; anything else is the exit code.  `constants` prints the program's "NAME value" lines.
int arguments(int argc, char **argv, const char *usage, void (*constants)(), Args &a) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) { constants(); return 0; }
    a.check = argc >= 3 && !strcmp(argv[1], "--check");
    if (argc < 3 || !strncmp(argv[a.check ? 2 : 1], "--", 2)) return fail(usage);
    a.in = argv[a.check ? 2 : 1];
    a.out = a.check ? nullptr : argv[2];
    a.n = argc - 3; a.v = argv + 3;
    return -1;
}

// ---- the case file: header[head] = magic, kind, njobs, the program's words; rows[njobs][8]; per job, in job order, two arrays
struct JobRow { int nUE, group, form, aT, nslots, E, lead, pad; }; // form: dist only; aT, nslots: log-record jobs; E, lead: the programs that say so
struct Place { size_t src_a, n_a, dst_a, src_b, n_b, dst_b; };     // in ints (src, n) and bytes (dst)

enum { E_UNUSED, E_PASSED, E_NOT_NEGATIVE }; // word 5 of a row: 0 to the kernel; handed on as it is; handed on and refused below 0

struct Rule {
    bool logs;         // the arrays: logs[nUE][16] and sched[nslots] (true), or dist's timers[nUE] and ptc[nUE] (form 0) / rec32[nUE][8] (form 1)
    int groups;        // a job's group is below this; 0: it is the job's index (a group is the offset of a store)
    int tile;          // wg0 is the running sum of ceil(nUE / tile); 0: the job's index, one workgroup per job
    int E;             // E_*
    long long max_ue;  // over all jobs
    bool trial_groups; // the device table names the job's index as its group, whatever the row says
};

struct Case {
    std::vector<int> w;  // the file, whole
    int head = 0, njobs = 0;
    const JobRow *rows = nullptr;
    std::vector<Place> pl;
    size_t arena = 0;    // bytes placed so far: a program with arrays of its own in the arena goes on from here, before stage()
    long long total_ue = 0;
    int wgs = 0, max_slots = 0;
    std::vector<unsigned char> staged;
    unsigned char *A = nullptr; // the arena on the device

    // The file, whole: length, alignment, short read, magic, kind (one of `kinds`), njobs, the job table.
    int read(const char *path, int head_words, std::initializer_list<int> kinds, long long max_jobs) {
        FILE *f = fopen(path, "rb");
        if (!f) return fail("cannot open the case file");
        fseek(f, 0, SEEK_END);
        const long fbytes = ftell(f);
        fseek(f, 0, SEEK_SET);
        if (fbytes < 4 * head_words || fbytes % 4) { fclose(f); return fail("case file: bad length"); }
        w.resize((size_t)fbytes / 4);
        const size_t got = fread(w.data(), 4, w.size(), f);
        fclose(f);
        if (got != w.size()) return fail("case file: short read");
        bool known = false;
        for (const int k : kinds) known |= w[1] == k;
        if (w[0] != MAGIC || !known) return fail("case file: bad header");
        head = head_words; njobs = w[2];
        if (njobs < 1 || njobs > max_jobs) return fail("case file: njobs out of range");
        if (w.size() < (size_t)head + 8 * (size_t)njobs) return fail("case file: job table cut short");
        rows = reinterpret_cast<const JobRow *>(w.data() + head);
        return 0;
    }

    // Every array of every job: checked against the file, placed at a 256-byte-aligned arena offset.
    int place(const Rule &rule) {
        pl.resize((size_t)njobs);
        size_t src = (size_t)head + 8 * (size_t)njobs;
        for (int j = 0; j < njobs; j++) {
            const JobRow &r = rows[j];
            if (r.nUE < 1 || (rule.groups ? r.group < 0 || r.group >= rule.groups : r.group != j)) return fail("job: nUE / group out of range");
            total_ue += r.nUE;
            if (total_ue > rule.max_ue) return fail("case file: too many UEs");
            size_t na = (size_t)r.nUE, nb = r.form ? 8 * (size_t)r.nUE : (size_t)r.nUE;
            if (rule.logs) {
                if (r.aT < 1 || r.nslots < 1 || r.nslots > (1 << 20) || (long long)r.aT * r.nslots > INT_MAX || (rule.E == E_NOT_NEGATIVE && r.E < 0))
                    return fail("job: aT / nslots / E out of range");
                if (r.nslots > max_slots) max_slots = r.nslots;
                na = 16 * (size_t)r.nUE; nb = (size_t)r.nslots;
            } else if (r.form != 0 && r.form != 1) return fail("job: form");
            if (rule.tile) wgs += (r.nUE + rule.tile - 1) / rule.tile;
            if (src + na + nb > w.size()) return fail("case file: arrays cut short");
            pl[(size_t)j] = Place{src, na, arena, src + na, nb, align256(arena + 4 * na)};
            arena = align256(pl[(size_t)j].dst_b + 4 * nb);
            src += na + nb;
            if (rule.logs) { // a schedule is non-decreasing and counts UEs of this trial: the kernels' searches assume it
                const int *const s = w.data() + pl[(size_t)j].src_b;
                for (int q = 0; q < r.nslots; q++)
                    if (s[q] < 0 || s[q] > r.nUE || (q && s[q] < s[q - 1])) return fail("job: schedule not a non-decreasing count of UEs");
            }
        }
        if (src != w.size()) return fail("case file: trailing data");
        return 0;
    }

    // The arena on the host, the gaps between the arrays at `fill` (a pattern, never zeros), then on the device.
    int upload(unsigned char fill = 0xA5) {
        stage(fill);
        CHK(hipMalloc(reinterpret_cast<void **>(&A), arena));
        CHK(hipMemcpy(A, staged.data(), arena, hipMemcpyHostToDevice));
        return 0;
    }
    void stage(unsigned char fill) {
        if (!staged.empty()) return; // (staged already, by a program that puts arrays of its own into it)
        staged.assign(arena, fill);
        for (const Place &p : pl) {
            memcpy(staged.data() + p.dst_a, w.data() + p.src_a, 4 * p.n_a);
            memcpy(staged.data() + p.dst_b, w.data() + p.src_b, 4 * p.n_b);
        }
    }

    // The device job table: make(row, a, b, group, wg0) is the kernel's job for one row, a and b its two arrays on the device.
    template <class Job, class Make>
    int table(const Rule &rule, Job *&dev, Make make) const {
        std::vector<Job> jobs((size_t)njobs);
        int wg0 = 0;
        for (int j = 0; j < njobs; j++) {
            jobs[(size_t)j] = make(rows[j], A + pl[(size_t)j].dst_a, A + pl[(size_t)j].dst_b, rule.trial_groups ? j : rows[j].group, rule.tile ? wg0 : j);
            if (rule.tile) wg0 += (rows[j].nUE + rule.tile - 1) / rule.tile;
        }
        CHK(hipMalloc(reinterpret_cast<void **>(&dev), sizeof(Job) * jobs.size()));
        CHK(hipMemcpy(dev, jobs.data(), sizeof(Job) * jobs.size(), hipMemcpyHostToDevice));
        return 0;
    }
    int timeline_table(const Rule &rule, prach::TimelineJob *&dev) const {
        return table(rule, dev, [&](const JobRow &r, const unsigned char *a, const unsigned char *b, int group, int wg0) {
            return prach::TimelineJob{reinterpret_cast<const int4 *>(a), reinterpret_cast<const int *>(b), r.nUE, group, wg0, r.aT, r.nslots, rule.E == E_UNUSED ? 0 : r.E};
        });
    }
};

// `n` 32-bit words of device memory, every one of them `pattern`.
template <class T>
int device_words(T *&p, size_t n, int pattern) {
    if (!n) return 0;
    CHK(hipMalloc(reinterpret_cast<void **>(&p), 4 * n));
    CHK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), pattern, n));
    return 0;
}

// The result file: the program's header words as they are, then the device bytes it names, in order.
struct Bytes { const void *dev; size_t n; };
int write_result(const char *path, const void *header, size_t header_bytes, std::initializer_list<Bytes> parts) {
    std::vector<unsigned char> res(header_bytes);
    memcpy(res.data(), header, header_bytes);
    for (const Bytes &b : parts) {
        if (!b.n) continue;
        res.resize(res.size() + b.n);
        CHK(hipMemcpy(res.data() + res.size() - b.n, b.dev, b.n, hipMemcpyDeviceToHost));
    }
    FILE *g = fopen(path, "wb");
    if (!g) return fail("cannot open the result file");
    const size_t put = fwrite(res.data(), 1, res.size(), g);
    if (fclose(g) != 0 || put != res.size()) return fail("result file: short write");
    return 0;
}

} // namespace
