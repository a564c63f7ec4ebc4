// tests/tools/gpu_stream_act_harness.hip — TEST INFRASTRUCTURE (GPU box): the device-side rand() stream generator (csrc/prach_stream.hip) and the device
// activeUE (csrc/prach_noma_act.h: noma_active_ue, near_float_boundary) away from every trial.  The case files come from tests/tools/stream_act_cases.py;
// the two product files are compiled into this program as they are, with the product's flags.  No product entry point is involved.
//
// usage: gpu_stream_act_harness CASE RESULT     one launch (the mode is in the case file); exit code 0 = launched, synchronised and written
//        gpu_stream_act_harness --constants     STREAM_CHUNK, ACT_BAND, ACT_GAIN_ULP_ASSERTED, NOMA_ACT_FLAG_CAP ... as compiled (no device needed)
//
// CASE (uint32, little endian): header[16] = magic, mode, n, ...; then
//   mode 1 `jobs`    n x job{n_lo, n_hi, nchunks, 0}, then per job, in job order, the seed windows [nchunks][31] (prach_internal_glibc_seeds with
//                    chunk = STREAM_CHUNK); ONE launch_glibc_stream_jobs over all of them, max_n = the longest
//   mode 2 `window`  the same layout with n = 1; ONE launch_glibc_stream
//   mode 3 `act`     header[3] = npool;  n x case{off, budget, cell radius (float bits), nP}, then pool[npool]: draw k of a case is pool[off + k], k < budget
// Modes 1, 2: ONE device arena, filled with the byte 0xA5; the StreamJob table, every job's windows and every job's output at 256-byte-aligned offsets of
// it, at least STREAM_GUARD_WORDS words behind every output before the next array begins.  The whole arena comes back.
// RESULT (uint32): modes 1, 2: header[8] = magic, mode, n, arena words, offset and length (words) of the StreamJob table, 0, 0; n x {seeds offset, output
//                  offset} (words); the arena
//                  mode 3: header[8] = magic, mode, n, 0 ...; n x {pre, sec, gain lo, hi, lgain lo, hi, flag, draws used, oob, 0}
// Mode 3 runs one thread per case in full wavefronts (the case table is padded with copies of case 0; every thread writes only its own ten words); draw()
// past the budget sets `oob` and returns 2147483647 / 3, as noma_glibc_trial_kernel's does.
#include "../../5g-nr-randomaccess_amd/csrc/prach_stream.hip"
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_act.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace prach {
namespace {

constexpr unsigned SA_MAGIC = 0x53414354u;
constexpr int SA_THREADS = 256;
constexpr size_t STREAM_GUARD_WORDS = 64;
constexpr size_t SA_MAX_JOBS = 1024, SA_MAX_STREAM_WORDS = 1u << 23, SA_MAX_CASES = 1u << 20, SA_MAX_POOL = 1u << 25;
constexpr int SA_ACT_WORDS = 10;

struct ActCase { unsigned off, budget, radius_bits, nP; };

__global__ __launch_bounds__(SA_THREADS) void act_kernel(const ActCase *__restrict__ cases, const int *__restrict__ pool, unsigned *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * SA_THREADS + threadIdx.x;
    const ActCase c = cases[gid];
    const int *const d = pool + c.off;
    unsigned used = 0;
    bool oob = false;
    const ActUe o = noma_active_ue([&]() -> int {
        const unsigned k = used++;
        if (k < c.budget) return d[k];
        oob = true;
        return 2147483647 / 3;
    }, (int)c.nP, __uint_as_float(c.radius_bits));
    const unsigned long long g = (unsigned long long)__double_as_longlong(o.gain), l = (unsigned long long)__double_as_longlong(o.lgain);
    unsigned *const w = out + SA_ACT_WORDS * gid;
    w[0] = (unsigned)o.pre; w[1] = (unsigned)o.sec; w[2] = (unsigned)g; w[3] = (unsigned)(g >> 32); w[4] = (unsigned)l; w[5] = (unsigned)(l >> 32);
    w[6] = o.flag ? 1u : 0u; w[7] = used; w[8] = oob ? 1u : 0u; w[9] = 0u;
}

#define CHK(call)                                                                                                 \
    do {                                                                                                          \
        const hipError_t rc_ = (call);                                                                            \
        if (rc_ != hipSuccess) {                                                                                  \
            fprintf(stderr, "gpu_stream_act_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                             \
        }                                                                                                         \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_stream_act_harness: %s\n", what);
    return 3;
}

int write_result(const char *path, const unsigned *head, const std::vector<unsigned> &a, const std::vector<unsigned> &b) {
    FILE *g = fopen(path, "wb");
    if (!g) return fail("cannot open the result file");
    size_t put = fwrite(head, 4, 8, g);
    if (!a.empty()) put += fwrite(a.data(), 4, a.size(), g);
    if (!b.empty()) put += fwrite(b.data(), 4, b.size(), g);
    if (fclose(g) != 0 || put != 8 + a.size() + b.size()) return fail("result file: short write");
    return 0;
}

size_t up256(const size_t bytes) { return (bytes + 255) / 256 * 256; }

int run_stream(const std::vector<unsigned> &w, const unsigned mode, const size_t n, const char *res_path) {
    if (n < 1 || n > SA_MAX_JOBS || (mode == 2 && n != 1)) return fail("stream: job count out of range");
    if (w.size() < 16 + 4 * n) return fail("stream: file length");
    const unsigned *tab = w.data() + 16;
    std::vector<unsigned long long> len(n);
    std::vector<size_t> nch(n), src(n), oseeds(n), oout(n);
    size_t at = 16 + 4 * n, total = 0;
    unsigned long long max_n = 0;
    size_t o = up256(sizeof(StreamJob) * n); // the job table first
    for (size_t j = 0; j < n; j++) {
        len[j] = (unsigned long long)tab[4 * j] | (unsigned long long)tab[4 * j + 1] << 32;
        nch[j] = tab[4 * j + 2];
        if (len[j] < 1 || len[j] > SA_MAX_STREAM_WORDS) return fail("stream: a job's length is out of range");
        if (nch[j] != (size_t)((len[j] + STREAM_CHUNK - 1) / STREAM_CHUNK)) return fail("stream: a job's window count is not that of its length");
        total += (size_t)len[j];
        if (total > SA_MAX_STREAM_WORDS) return fail("stream: too many values");
        src[j] = at;
        at += 31 * nch[j];
        if (len[j] > max_n) max_n = len[j];
        oseeds[j] = o; o = up256(o + 4 * 31 * nch[j]);
        oout[j] = o; o = up256(o + 4 * ((size_t)len[j] + STREAM_GUARD_WORDS));
    }
    if (at != w.size()) return fail("stream: file length");
    const size_t arena = o;
    unsigned char *d = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&d), arena));
    CHK(hipMemset(d, 0xA5, arena));
    std::vector<StreamJob> jobs(n);
    for (size_t j = 0; j < n; j++) {
        CHK(hipMemcpy(d + oseeds[j], w.data() + src[j], 4 * 31 * nch[j], hipMemcpyHostToDevice));
        jobs[j] = StreamJob{reinterpret_cast<const unsigned *>(d + oseeds[j]), reinterpret_cast<int *>(d + oout[j]), len[j]};
    }
    CHK(hipMemcpy(d, jobs.data(), sizeof(StreamJob) * n, hipMemcpyHostToDevice));
    if (mode == 1) CHK(launch_glibc_stream_jobs(reinterpret_cast<const StreamJob *>(d), (int)n, max_n, nullptr));
    else CHK(launch_glibc_stream(jobs[0].seeds, jobs[0].out, len[0], nullptr));
    CHK(hipDeviceSynchronize());
    std::vector<unsigned> back(arena / 4), layout(2 * n);
    CHK(hipMemcpy(back.data(), d, arena, hipMemcpyDeviceToHost));
    CHK(hipFree(d));
    for (size_t j = 0; j < n; j++) { layout[2 * j] = (unsigned)(oseeds[j] / 4); layout[2 * j + 1] = (unsigned)(oout[j] / 4); }
    const unsigned head[8] = {SA_MAGIC, mode, (unsigned)n, (unsigned)(arena / 4), 0u, (unsigned)(sizeof(StreamJob) * n / 4), 0u, 0u};
    return write_result(res_path, head, layout, back);
}

int run_act(const std::vector<unsigned> &w, const size_t n, const char *res_path) {
    const size_t npool = w[3];
    if (n < 1 || n > SA_MAX_CASES || npool < 1 || npool > SA_MAX_POOL || w.size() != 16 + 4 * n + npool) return fail("act: file length");
    const ActCase *tab = reinterpret_cast<const ActCase *>(w.data() + 16);
    for (size_t k = 0; k < n; k++) {
        float radius;
        memcpy(&radius, &tab[k].radius_bits, 4);
        if ((size_t)tab[k].off > npool || (size_t)tab[k].budget > npool - tab[k].off) return fail("act: a case's draws leave the pool");
        if (tab[k].nP < 1 || tab[k].nP > 65536 || !(radius > 35.0f) || !(radius < 1e6f)) return fail("act: preamble count / cell radius out of range");
    }
    for (size_t k = 0; k < npool; k++)
        if (w[16 + 4 * n + k] > 2147483647u) return fail("act: a draw is never negative");
    const size_t npad = (n + SA_THREADS - 1) / SA_THREADS * SA_THREADS;
    std::vector<ActCase> cases(npad, tab[0]); // whole wavefronts: copies of case 0
    memcpy(cases.data(), tab, sizeof(ActCase) * n);
    ActCase *dc = nullptr;
    int *dp = nullptr;
    unsigned *dout = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&dc), sizeof(ActCase) * npad));
    CHK(hipMalloc(reinterpret_cast<void **>(&dp), 4 * npool));
    CHK(hipMalloc(reinterpret_cast<void **>(&dout), 4 * SA_ACT_WORDS * npad));
    CHK(hipMemcpy(dc, cases.data(), sizeof(ActCase) * npad, hipMemcpyHostToDevice));
    CHK(hipMemcpy(dp, w.data() + 16 + 4 * n, 4 * npool, hipMemcpyHostToDevice));
    CHK(hipMemset(dout, 0xA5, 4 * SA_ACT_WORDS * npad));
    hipLaunchKernelGGL(act_kernel, dim3((unsigned)(npad / SA_THREADS)), dim3(SA_THREADS), 0, nullptr, dc, dp, dout);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    std::vector<unsigned> body(SA_ACT_WORDS * n);
    CHK(hipMemcpy(body.data(), dout, 4 * body.size(), hipMemcpyDeviceToHost));
    CHK(hipFree(dc));
    CHK(hipFree(dp));
    CHK(hipFree(dout));
    const unsigned head[8] = {SA_MAGIC, 3u, (unsigned)n, 0u, 0u, 0u, 0u, 0u};
    return write_result(res_path, head, body, {});
}

int read_words(const char *path, std::vector<unsigned> &w) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail("cannot open the case file");
    fseek(f, 0, SEEK_END);
    const long fbytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fbytes < 64 || fbytes % 4) { fclose(f); return fail("case file: bad length"); }
    w.resize((size_t)fbytes / 4);
    const size_t got = fread(w.data(), 4, w.size(), f);
    fclose(f);
    if (got != w.size()) return fail("case file: short read");
    if (w[0] != SA_MAGIC || w[1] < 1 || w[1] > 3) return fail("case file: bad header");
    return 0;
}

} // namespace
} // namespace prach

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("STREAM_CHUNK %d\nACT_BAND %lld\nACT_GAIN_ULP_ASSERTED %d\nNOMA_ACT_FLAG_CAP %d\n", STREAM_CHUNK, ACT_BAND, ACT_GAIN_ULP_ASSERTED, NOMA_ACT_FLAG_CAP);
        printf("STREAM_GUARD_WORDS %zu\nSTREAM_JOB_BYTES %zu\nSA_ACT_WORDS %d\nSA_THREADS %d\n", STREAM_GUARD_WORDS, sizeof(StreamJob), SA_ACT_WORDS, SA_THREADS);
        return 0;
    }
    if (argc != 3) return fail("usage: gpu_stream_act_harness CASE RESULT | --constants");
    std::vector<unsigned> w;
    const int rc = read_words(argv[1], w);
    if (rc) return rc;
    return w[1] == 3 ? run_act(w, w[2], argv[2]) : run_stream(w, w[1], w[2], argv[2]);
}
