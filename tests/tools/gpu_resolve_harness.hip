// tests/tools/gpu_resolve_harness.hip — TEST INFRASTRUCTURE (GPU box): the device code that decides who gets a grant, away from every trial.  The case
// files come from tests/tools/resolve_cases.py: singleton sets, gains, draw tables and event lists no Monte-Carlo trial produces.  The product's headers
// and prach_noma_glibc.hip are compiled into this program as they are (build it with the product's -ffp-contract=off); no product entry point is involved.
//   mode 1  prach::noma_resolve_sector (prach_noma_resolve.h) in a wrapper kernel: one wavefront (= one workgroup of 64) per case, the staging arrays in
//           LDS, the count <= nGrantUL shortcut stated as its caller states it (prach_noma.hip)
//   mode 2  the restatement inside prach::noma_glibc_slot (prach_noma_glibc.hip, anonymous namespace: this file includes it) in a wrapper kernel with the
//           LDS arrays of noma_glibc_slot_kernel: one workgroup of WG_THREADS per case, one access slot (subframe 0) of synthetic NUe records that are all
//           due to transmit.  maxRarWindow = 6 and stop = 0: msg2Results then draws nothing and never touches msg2 (rar_expires is false, `need` stays 0),
//           and the slot's subframe loop does not run (time + k < stop is false), so msg2, the stream position and the status are the grouping's alone.
//           (noma_glibc_slot_kernel itself takes one trial per launch and fixes devact = false; thousands of cases want one launch and both values.)
//   mode 3  prach::classify_event by a whole workgroup, then prach::resolve_reset_candidates<1 | 4> by wavefront 0 when nrc <= RCCAP (prach_resolve.h),
//           the tables in LDS, one workgroup of 256 per case
//
// usage: gpu_resolve_harness CASE RESULT DEVACT     ONE launch; exit code 0 = launched, synchronised and written; anything else is an error (stderr)
//        gpu_resolve_harness --constants            compile-time constants, one "NAME value" per line (no device needed)
//
// CASE (int32, little endian): header[16] = magic, mode, ncases, 0 ...; then
//   mode 1  per case M1_WORDS: nGrantUL, nonsector, budget, 0, idx[64] (lane = preamble: the UE index 0..63 of its only transmitter, or -1),
//           draws[64][2] (grant, which), gain[64], lgain[64] (doubles, by UE index)
//   mode 2  table[ncases][8] = nUE, nP, nGrantUL, nonsector, pos0, budget, nstream, 0; then per case ue[nUE][8] = sector, preamble, 0, 0, gain, lgain
//           (doubles) and stream[nstream] (the kernel's stream_len is pos0 + budget <= nstream)
//   mode 3  table[ncases][8] = nP, NB, nev, 0 ...; then per case fcall[nP], events[nev][2] = idx, info
// RESULT (int32): header[4] = magic, mode, devact, ncases; then
//   mode 1  per case M1_RES: granted[64] (by UE index), ntaken, taken[128] (2 grant + which, in order), status, ambiguous, 0
//   mode 2  per case msg2[nUE], pos (relative to pos0), status, 0, 0
//   mode 3  per case nrc, nrj, resolved, 0, fcall[nP], nlv[nP], fie[nP], void[nev]
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_glibc.hip"
#include "../../5g-nr-randomaccess_amd/csrc/prach_noma_resolve.h"
#include "../../5g-nr-randomaccess_amd/csrc/prach_resolve.h"

#include <cstdlib>

// host-side externals of prach_noma_glibc.hip's staging and launch functions, which this program never calls
extern "C" int prach_arrival_schedule(const prach_cfg *, int32_t *, int, int32_t *) { abort(); }
extern "C" int prach_noma_activation_stream(const prach_cfg *, const int32_t *, uint64_t *, uint64_t, int32_t *, int32_t *, double *, double *) { abort(); }
extern "C" void prach_internal_glibc_seeds(uint32_t, uint64_t, uint64_t, uint64_t, uint32_t *) { abort(); }
namespace prach {
hipError_t launch_glibc_stream_jobs(const StreamJob *, int, unsigned long long, hipStream_t) { abort(); }
} // namespace prach

namespace prach {
namespace {

constexpr int MAGIC = 0x52534c56;
constexpr int M1_WORDS = 4 + 64 + 128 + 128 + 128, M1_IDX = 4, M1_DRAWS = 68, M1_GAIN = 196, M1_LGAIN = 324;
constexpr int M1_RES = 196, M1_NTAKEN = 64, M1_TAKEN = 65, M1_STATUS = 193, M1_AMBIG = 194;
constexpr int M3_THREADS = 256, M3_MAX_EVENTS = 1 << 14;
constexpr int MAX_CASES = 1 << 16;

// ---- mode 1 ----
__global__ __launch_bounds__(64) void shared_copy_kernel(const int *__restrict__ cases, int *__restrict__ out, const int devact) {
    __shared__ int sidx[64];
    __shared__ double sg[64], slg[64];
    const int *const c = cases + (size_t)blockIdx.x * M1_WORDS;
    int *const o = out + (size_t)blockIdx.x * M1_RES;
    const int lane = threadIdx.x;
    const int nGrantUL = c[0], budget = c[2];
    const bool nonsector = c[1] != 0;
    const int myidx = c[M1_IDX + lane];
    const bool single = myidx >= 0;
    const double *const gain = reinterpret_cast<const double *>(c + M1_GAIN), *const lgain = reinterpret_cast<const double *>(c + M1_LGAIN);
    const int count = __popcll(__ballot(single));
    int taken = 0, status = PRACH_OK;
    bool ambiguous = false;
    if (count > 0 && count <= nGrantUL) { // the caller's shortcut (prach_noma.hip; NOMA.c:245-250)
        if (single) o[myidx] = 1;
    } else if (count > 0) {
        const NomaResolved R = noma_resolve_sector(single, myidx, nGrantUL, nonsector, devact, sidx, sg, slg,
            [&](const int idx) __attribute__((always_inline)) { return NomaGain{gain[idx], lgain[idx]}; },
            [&](const int g, const int which, int &d) __attribute__((always_inline)) {
                if (taken >= budget) return false;
                d = c[M1_DRAWS + 2 * g + which];
                if (lane == 0 && taken < 128) o[M1_TAKEN + taken] = 2 * g + which;
                taken++;
                return true;
            },
            [&](const int idx) __attribute__((always_inline)) { o[idx] = 1; },
            [&](const int) __attribute__((always_inline)) {});
        status = R.status; ambiguous = R.ambiguous;
    }
    if (lane == 0) { o[M1_NTAKEN] = taken; o[M1_STATUS] = status; o[M1_AMBIG] = ambiguous ? 1 : 0; }
}

// ---- mode 2 ----
struct G2Case { NUe *ue; const int *stream; unsigned long long pos0, slen; NParams K; int pad; };

__global__ __launch_bounds__(WG_THREADS) void glibc_copy_kernel(const G2Case *__restrict__ cases, int *__restrict__ out, const int devact) {
    __shared__ int cnt[6 * 64], who[6 * 64], wtot[NW], sh[8], gs_idx[64]; // (as noma_glibc_slot_kernel)
    __shared__ double gs_g[64], gs_lg[64];
    const G2Case A = cases[blockIdx.x];
    unsigned long long pos = A.pos0;
    int status = PRACH_OK, exit_time = -1, nsucc = 0;
    noma_glibc_slot((NG NUe *)A.ue, (const NG int *)A.stream, A.K, cnt, who, wtot, sh, gs_idx, gs_g, gs_lg, 0, A.K.nUE, nullptr, 0, 0, A.slen, devact != 0, pos, status,
                    exit_time, nsucc);
    if (threadIdx.x == 0) {
        int *const o = out + 4 * (size_t)blockIdx.x;
        o[0] = (int)(pos - A.pos0); o[1] = status; o[2] = exit_time; o[3] = nsucc;
    }
}

// ---- mode 3 ----
struct R3Case { const int *fcall; const int2 *ev; int *out; int nP, NB, nev, pad; };

__global__ __launch_bounds__(M3_THREADS) void reset_candidates_kernel(const R3Case *__restrict__ cases) {
    __shared__ int fcall[256], nlv[256], fie[256], rclist[RCCAP], sidx[RCCAP], scal[2];
    const R3Case A = cases[blockIdx.x];
    const int tid = threadIdx.x, nP = A.nP, nev = A.nev;
    int *const o = A.out, *const o_void = A.out + 4 + 3 * nP;
    for (int k = tid; k < 256; k += M3_THREADS) { fcall[k] = k < nP ? A.fcall[k] : INT_MAX; nlv[k] = 0; fie[k] = 0; }
    for (int k = tid; k < RCCAP; k += M3_THREADS) { rclist[k] = 0; sidx[k] = 0; }
    if (tid < 2) scal[tid] = 0;
    __syncthreads();
    const ResolveTables RT{fcall, nlv, fie, rclist, sidx, &scal[0], &scal[1]};
    auto get = [&](const int k) __attribute__((always_inline)) -> int2 { return A.ev[k]; };
    auto kill = [&](const int k) __attribute__((always_inline)) { o_void[k] = 1; };
    for (int k = tid; k < nev; k += M3_THREADS) classify_event(RT, k, get(k), kill);
    __syncthreads();
    const int nrc = scal[0];
    if (nrc <= RCCAP && tid < 64) {
        if (A.NB == 1) resolve_reset_candidates<1>(RT, nrc, nP, get, kill);
        else resolve_reset_candidates<4>(RT, nrc, nP, get, kill);
    }
    __syncthreads();
    if (tid == 0) { o[0] = nrc; o[1] = scal[1]; o[2] = nrc <= RCCAP ? 1 : 0; }
    for (int k = tid; k < nP; k += M3_THREADS) { o[4 + k] = fcall[k]; o[4 + nP + k] = nlv[k]; o[4 + 2 * nP + k] = fie[k]; }
}

#define CHK(call)                                                                                              \
    do {                                                                                                       \
        const hipError_t rc_ = (call);                                                                         \
        if (rc_ != hipSuccess) {                                                                               \
            fprintf(stderr, "gpu_resolve_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                          \
        }                                                                                                      \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_resolve_harness: %s\n", what);
    return 3;
}

int write_result(const char *path, const int mode, const int devact, const int ncases, const std::vector<int> &body) {
    std::vector<int> res(4 + body.size());
    res[0] = MAGIC; res[1] = mode; res[2] = devact; res[3] = ncases;
    if (!body.empty()) memcpy(res.data() + 4, body.data(), 4 * body.size());
    FILE *g = fopen(path, "wb");
    if (!g) return fail("cannot open the result file");
    const size_t put = fwrite(res.data(), 4, res.size(), g);
    if (fclose(g) != 0 || put != res.size()) return fail("result file: short write");
    return 0;
}

int run_mode1(const std::vector<int> &w, const int ncases, const int devact, const char *res_path) {
    if (w.size() != 16 + (size_t)ncases * M1_WORDS) return fail("mode 1: file length");
    for (int k = 0; k < ncases; k++) { // every index the kernel forms stays inside the case's record
        const int *c = w.data() + 16 + (size_t)k * M1_WORDS;
        if (c[0] < 1 || c[0] > 64 || c[2] < 0) return fail("mode 1: nGrantUL / budget out of range");
        unsigned long long seen = 0;
        for (int l = 0; l < 64; l++) {
            const int i = c[M1_IDX + l];
            if (i < -1 || i > 63) return fail("mode 1: UE index out of range");
            if (i >= 0) { if ((seen >> i) & 1ull) return fail("mode 1: UE index twice"); seen |= 1ull << i; }
        }
    }
    int *dc = nullptr, *dout = nullptr;
    const size_t cbytes = 4 * (size_t)ncases * M1_WORDS, obytes = 4 * (size_t)ncases * M1_RES;
    CHK(hipMalloc(reinterpret_cast<void **>(&dc), cbytes));
    CHK(hipMalloc(reinterpret_cast<void **>(&dout), obytes));
    CHK(hipMemcpy(dc, w.data() + 16, cbytes, hipMemcpyHostToDevice));
    CHK(hipMemset(dout, 0, obytes));
    hipLaunchKernelGGL(shared_copy_kernel, dim3((unsigned)ncases), dim3(64), 0, nullptr, dc, dout, devact);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    std::vector<int> body((size_t)ncases * M1_RES);
    CHK(hipMemcpy(body.data(), dout, obytes, hipMemcpyDeviceToHost));
    return write_result(res_path, 1, devact, ncases, body);
}

int run_mode2(const std::vector<int> &w, const int ncases, const int devact, const char *res_path) {
    if (w.size() < 16 + 8 * (size_t)ncases) return fail("mode 2: case table cut short");
    const int *const tab = w.data() + 16;
    std::vector<NUe> ue;
    std::vector<int> stream;
    std::vector<size_t> ue0((size_t)ncases), st0((size_t)ncases);
    size_t src = 16 + 8 * (size_t)ncases;
    for (int k = 0; k < ncases; k++) {
        const int *t = tab + 8 * (size_t)k;
        const int nUE = t[0], nP = t[1], nG = t[2], pos0 = t[4], budget = t[5], nstream = t[6];
        if (nUE < 1 || nUE > 4096 || nP < 1 || nP > 64 || nG < 1 || nG > 64) return fail("mode 2: nUE / nP / nGrantUL out of range");
        if (pos0 < 0 || budget < 0 || nstream < 0 || nstream > (1 << 16) || (long long)pos0 + budget > nstream) return fail("mode 2: stream window out of range");
        if (src + 8 * (size_t)nUE + (size_t)nstream > w.size()) return fail("mode 2: arrays cut short");
        ue0[(size_t)k] = ue.size(); st0[(size_t)k] = stream.size();
        for (int i = 0; i < nUE; i++) {
            const int *r = w.data() + src + 8 * (size_t)i;
            if (r[0] < 0 || r[0] > 5 || r[1] < 0 || r[1] >= nP) return fail("mode 2: sector / preamble out of range");
            NUe u;
            memset(&u, 0, sizeof u);
            u.active = 1; u.txTime = 1; u.firstTxTime = 1; u.nTxPreamble = 1; u.sector = r[0]; u.preamble = r[1]; // due in the slot of subframe 0
            memcpy(&u.gain, r + 4, 8); memcpy(&u.lgain, r + 6, 8);
            ue.push_back(u);
        }
        src += 8 * (size_t)nUE;
        stream.insert(stream.end(), w.begin() + (long)src, w.begin() + (long)(src + (size_t)nstream));
        src += (size_t)nstream;
    }
    if (src != w.size()) return fail("mode 2: trailing data");
    stream.push_back(0);
    NUe *due = nullptr;
    int *dstream = nullptr, *dout = nullptr;
    G2Case *dcases = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&due), sizeof(NUe) * ue.size()));
    CHK(hipMalloc(reinterpret_cast<void **>(&dstream), 4 * stream.size()));
    CHK(hipMalloc(reinterpret_cast<void **>(&dout), 16 * (size_t)ncases));
    CHK(hipMalloc(reinterpret_cast<void **>(&dcases), sizeof(G2Case) * (size_t)ncases));
    std::vector<G2Case> cs((size_t)ncases);
    for (int k = 0; k < ncases; k++) {
        const int *t = tab + 8 * (size_t)k;
        cs[(size_t)k] = G2Case{due + ue0[(size_t)k], dstream + st0[(size_t)k], (unsigned long long)t[4], (unsigned long long)t[4] + (unsigned long long)t[5],
                               NParams{t[0], t[1], 20, t[2], 6, 10, 5, 0, t[3] ? 1 : 0}, 0};
    }
    CHK(hipMemcpy(due, ue.data(), sizeof(NUe) * ue.size(), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dstream, stream.data(), 4 * stream.size(), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dcases, cs.data(), sizeof(G2Case) * cs.size(), hipMemcpyHostToDevice));
    CHK(hipMemset(dout, 0, 16 * (size_t)ncases));
    hipLaunchKernelGGL(glibc_copy_kernel, dim3((unsigned)ncases), dim3(WG_THREADS), 0, nullptr, dcases, dout, devact);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    std::vector<int> o4(4 * (size_t)ncases), body;
    CHK(hipMemcpy(ue.data(), due, sizeof(NUe) * ue.size(), hipMemcpyDeviceToHost));
    CHK(hipMemcpy(o4.data(), dout, 16 * (size_t)ncases, hipMemcpyDeviceToHost));
    for (int k = 0; k < ncases; k++) {
        const int nUE = tab[8 * (size_t)k];
        for (int i = 0; i < nUE; i++) body.push_back(ue[ue0[(size_t)k] + (size_t)i].msg2);
        body.push_back(o4[4 * (size_t)k]); body.push_back(o4[4 * (size_t)k + 1]); body.push_back(0); body.push_back(0);
        if (o4[4 * (size_t)k + 2] != -1 || o4[4 * (size_t)k + 3] != 0) return fail("mode 2: the slot's subframe loop ran");
    }
    return write_result(res_path, 2, devact, ncases, body);
}

int run_mode3(const std::vector<int> &w, const int ncases, const char *res_path) {
    if (w.size() < 16 + 8 * (size_t)ncases) return fail("mode 3: case table cut short");
    const int *const tab = w.data() + 16;
    std::vector<size_t> in0((size_t)ncases), out0((size_t)ncases);
    size_t src = 16 + 8 * (size_t)ncases, outw = 0;
    for (int k = 0; k < ncases; k++) {
        const int *t = tab + 8 * (size_t)k;
        const int nP = t[0], NB = t[1], nev = t[2];
        if ((NB != 1 && NB != 4) || nP < 1 || nP > (NB == 1 ? 64 : 256) || nev < 0 || nev > M3_MAX_EVENTS) return fail("mode 3: nP / NB / nev out of range");
        if (src + (size_t)nP + 2 * (size_t)nev > w.size()) return fail("mode 3: arrays cut short");
        const int *e = w.data() + src + nP;
        for (int q = 0; q < nev; q++) {
            const int idx = e[2 * q], info = e[2 * q + 1];
            if (idx < 0 || idx >= (1 << 20) || (info >> 20) != 0 || ((info >> 4) & 0xff) >= nP || ((info >> 12) & 0xff) >= nP) return fail("mode 3: event out of range");
        }
        in0[(size_t)k] = src - 16 - 8 * (size_t)ncases; out0[(size_t)k] = outw;
        src += (size_t)nP + 2 * (size_t)nev;
        outw += 4 + 3 * (size_t)nP + (size_t)nev;
    }
    if (src != w.size()) return fail("mode 3: trailing data");
    int *din = nullptr, *dout = nullptr;
    R3Case *dcases = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&dout), 4 * outw));
    CHK(hipMalloc(reinterpret_cast<void **>(&dcases), sizeof(R3Case) * (size_t)ncases));
    // (an event is read as one int2: fcall tables of odd length would leave the list behind them at an odd word, so every case's list is staged 8-byte aligned)
    std::vector<int> stage;
    std::vector<R3Case> cs((size_t)ncases);
    std::vector<size_t> f0((size_t)ncases), e0((size_t)ncases);
    for (int k = 0; k < ncases; k++) {
        const int *t = tab + 8 * (size_t)k;
        const int *p = w.data() + 16 + 8 * (size_t)ncases + in0[(size_t)k];
        f0[(size_t)k] = stage.size();
        stage.insert(stage.end(), p, p + t[0]);
        if (stage.size() & 1) stage.push_back(0);
        e0[(size_t)k] = stage.size();
        stage.insert(stage.end(), p + t[0], p + t[0] + 2 * (size_t)t[2]);
    }
    CHK(hipMalloc(reinterpret_cast<void **>(&din), 4 * (stage.size() + 2)));
    for (int k = 0; k < ncases; k++) {
        const int *t = tab + 8 * (size_t)k;
        cs[(size_t)k] = R3Case{din + f0[(size_t)k], reinterpret_cast<const int2 *>(din + e0[(size_t)k]), dout + out0[(size_t)k], t[0], t[1], t[2], 0};
    }
    CHK(hipMemcpy(din, stage.data(), 4 * stage.size(), hipMemcpyHostToDevice));
    CHK(hipMemcpy(dcases, cs.data(), sizeof(R3Case) * cs.size(), hipMemcpyHostToDevice));
    CHK(hipMemset(dout, 0, 4 * outw));
    hipLaunchKernelGGL(reset_candidates_kernel, dim3((unsigned)ncases), dim3(M3_THREADS), 0, nullptr, dcases);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    std::vector<int> body(outw);
    CHK(hipMemcpy(body.data(), dout, 4 * outw, hipMemcpyDeviceToHost));
    return write_result(res_path, 3, 0, ncases, body);
}

} // namespace
} // namespace prach

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("UEV_NONE %d\nUEV_CALLER %d\nUEV_RESETCAND %d\nUEV_RJOIN %d\nEV_LEAVER %d\nRCCAP %d\nWG_THREADS %d\nPRACH_OK %d\nPRACH_ERR_STREAM %d\n"
               "NOMA_GLIBC_AMBIGUOUS %d\nNUE_BYTES %d\nM1_WORDS %d\nM1_RES %d\nACT_GAIN_ORDER_BAND %a\n",
               UEV_NONE, UEV_CALLER, UEV_RESETCAND, UEV_RJOIN, EV_LEAVER, RCCAP, WG_THREADS, PRACH_OK, PRACH_ERR_STREAM, NOMA_GLIBC_AMBIGUOUS, (int)sizeof(NUe), M1_WORDS,
               M1_RES, ACT_GAIN_ORDER_BAND);
        return 0;
    }
    if (argc != 4) return fail("usage: gpu_resolve_harness CASE RESULT DEVACT | --constants");
    const int devact = atoi(argv[3]);
    if (devact < 0 || devact > 2) return fail("devact out of range");
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    fseek(f, 0, SEEK_END);
    const long fbytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fbytes < 64 || fbytes % 4) { fclose(f); return fail("case file: bad length"); }
    std::vector<int> w((size_t)fbytes / 4);
    const size_t got = fread(w.data(), 4, w.size(), f);
    fclose(f);
    if (got != w.size()) return fail("case file: short read");
    const int mode = w[1], ncases = w[2];
    if (w[0] != MAGIC || mode < 1 || mode > 3 || ncases < 1 || ncases > MAX_CASES) return fail("case file: bad header");
    if (mode == 2 && devact == 2) return fail("mode 2 has no devact 2");
    if (mode == 3 && devact != 0) return fail("mode 3 takes devact 0");
    if (mode == 1) return run_mode1(w, ncases, devact, argv[2]);
    if (mode == 2) return run_mode2(w, ncases, devact, argv[2]);
    return run_mode3(w, ncases, argv[2]);
}
