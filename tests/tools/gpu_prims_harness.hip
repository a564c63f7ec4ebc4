// tests/tools/gpu_prims_harness.hip — TEST INFRASTRUCTURE (GPU box): the small __device__ building blocks every trial kernel is made of, away from every
// trial.  The case files come from tests/tools/prims_cases.py.  The product's headers and prach_cluster.hip (for the record helpers in its anonymous
// namespace) are compiled into this program as they are, with the product's flags; it is built a second time with the NOBITOP3 flags of csrc/Makefile, and
// every section's output must be the same under both.  No product entry point is involved, and no kernel here waits for another workgroup (wait_granule
// and same_xcd_handshake are never called).
//   1 philox   philox_draw31, philox_draw31_x2                                   one case per thread
//   2 masks    pass_masks<false>, pass_masks<true>, light_case                    one record per lane, one 64-record group per wavefront
//   3 wave     wave_scan_incl, wave_sum, wave_max                                 one row of 64 per wavefront
//   4 mod      fastmod, fastmod_flat, slot_align_fm, slot_align_flat, slot_align  one case per thread
//   5 sector   sector_of_draw                                                     one draw per thread
//   6 granule  mk_granule, granule_ok                                             one case per thread
//   7 blocks   cluster_block                                                      one launch per (G, xpack, ntrials, grid), 64 threads per block
//   8 hot      hot_encode / hot_decode / hot_fits, then slot_of / idx_of          two launches
//   9 pack     pack / unpack                                                      --host only
// Every wrapper kernel runs full 64-lane wavefronts only (the DPP primitives and pass_masks need all lanes active): the host pads the case arrays with
// copies of the first case, no lane is guarded off.  Every thread writes only out[its own global id].
//
// usage: gpu_prims_harness SECTION CASE RESULT          the section's launch(es); exit code 0 = launched, synchronised and written; anything else is an error
//        gpu_prims_harness --host SECTION CASE RESULT   sections 2, 4, 9 on the CPU, no device: whatever is host-callable (the branched body is the masks' reference)
//        gpu_prims_harness --constants                  compile-time constants, one "NAME value" per line (no device needed)
//
// CASE (int32, little endian): header[16] = magic, section, n, p3, p4 ...; then
//   1  n x {k0, k1, c0, c1, c2, c3}
//   2  p3 = maxMsg2;  n / 64 x group{t, maxRar, front, i0, acNow, acPrev, nUE, 0};  n x rec{kind, a, b, c}: kind 0: record a of the enumeration of
//      (t, maxRar) (prims_decode below, shared by the kernel and --host); kind 1: the raw record txTime a, nowBackoff b, packed word c
//   3  n x row[64]
//   4  n x {x, d, sub, aT}
//   5  n x {d}
//   6  n x {kind, a, b, tag, probe}: kind 0: g = mk_granule(a, b, tag); kind 1: g = the words a, b as they are
//   7  n x {G, xpack, ntrials, grid}
//   8  p3 = nslotpairs, p4 = lslots;  n x {tx, bo, pk};  p3 x {G, b}
//   9  n x {tx, tb, bo, pk}
// RESULT (uint32): header[4] = magic, section, host (0 / 1), n; then per case / thread
//   1  d, d1, d2, 0                      2 (device)  one word of mask bits: light, quiet, done, trig of <false> (bits 0-3), of <true> (4-7), light_case (8)
//   2 (--host)  flags, tx, bo, pk after the body, rx, rz, pk before it, tb after it; flags: applied 1, dirty 2, need << 2, evtype << 4, cold field
//      touched 128, counter touched 256
//   3  per lane scan, sum, max, 0        4  fastmod, fastmod_flat, slot_align_fm, slot_align_flat, slot_align, M, 0, 0       5  sector
//   6  w0, w1, granule_ok(g, tag), granule_ok(g, probe)
//   7  per thread (grid x 64 per set): ok << 31 | unpackable << 30 | T << 8 | b
//   8  n x {h.x, h.y, decoded tx, decoded bo, decoded pk, decoded tb, fits, 0}, then p3 x lslots x {idx_of(slot), slot_of(idx_of(slot))}
//   9  tx, tb, bo, act, conn, pre, rar, mrc, pend, pack(unpack(r)).w, and x, y, z of the re-packed record: 13 words
#include "../../5g-nr-randomaccess_amd/csrc/prach_device_fn.h"
#include "../../5g-nr-randomaccess_amd/csrc/prach_ue_body.h"
#include "../../5g-nr-randomaccess_amd/csrc/prach_exchange.h"
#include "../../5g-nr-randomaccess_amd/csrc/prach_cluster.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace prach {
namespace {

constexpr int PRIMS_MAGIC = 0x50524d53;
constexpr int PRIMS_THREADS = 256;
constexpr int PRIMS_TB_BACK = 50;          // the timer base of an enumerated record: t - 50
constexpr size_t PRIMS_MAX_THREADS = 1u << 24;
constexpr int PRIMS_MAX_GRID7 = 1 << 17;

// ---- the record enumeration of section 2: ONE function for the kernel and for --host ------------------------------------------------------------------
// digits, fastest first: rz {-2, 0, 1, t - 1, t, t + 1, t + 5}, rx t - 4 .. t + 2, grant, pend 0..5, mrc {0, maxMsg2, maxMsg2 + 1}, rar 0 .. maxRar + 1,
// pre {0, 1, 5, 255}, conn 0..2, act 0..3
PRACH_HD unsigned prims_enum_size(const int maxRar) { return 7u * 7u * 2u * 6u * 3u * (unsigned)(maxRar + 2) * 4u * 3u * 4u; }
struct PrimRec { int rx, rz; unsigned pk; };
PRACH_HD PrimRec prims_decode(unsigned e, const int t, const int maxRar, const int maxMsg2) {
    const int krz = (int)(e % 7u); e /= 7u;
    const int krx = (int)(e % 7u); e /= 7u;
    const unsigned grant = e % 2u; e /= 2u;
    const unsigned pend = e % 6u; e /= 6u;
    const int kmrc = (int)(e % 3u); e /= 3u;
    const unsigned rar = e % (unsigned)(maxRar + 2); e /= (unsigned)(maxRar + 2);
    const int kpre = (int)(e % 4u); e /= 4u;
    const unsigned conn = e % 3u; e /= 3u;
    const unsigned act = e % 4u;
    PrimRec r;
    r.rz = krz == 0 ? -2 : krz == 1 ? 0 : krz == 2 ? 1 : krz == 3 ? t - 1 : krz == 4 ? t : krz == 5 ? t + 1 : t + 5;
    r.rx = t - 4 + krx;
    const unsigned pre = kpre == 0 ? 0u : kpre == 1 ? 1u : kpre == 2 ? 5u : 255u;
    const unsigned mrc = kmrc == 0 ? 0u : (unsigned)(maxMsg2 + kmrc - 1);
    r.pk = (act << PK_ACT_SHIFT) | (conn << PK_CONN_SHIFT) | (pre << PK_PRE_SHIFT) | (rar << PK_RAR_SHIFT) | (mrc << PK_MRC_SHIFT) | (pend << PK_PEND_SHIFT) |
           (grant ? PK_GRANT_BIT : 0u);
    return r;
}
PRACH_HD PrimRec prims_record(const int *rec, const int t, const int maxRar, const int maxMsg2) {
    if (rec[0] == 0) return prims_decode((unsigned)rec[1], t, maxRar, maxMsg2);
    PrimRec r;
    r.rx = rec[1]; r.rz = rec[2]; r.pk = (unsigned)rec[3];
    return r;
}

// ---- section 1 ----
__global__ __launch_bounds__(PRIMS_THREADS) void philox_kernel(const unsigned *__restrict__ c, uint4 *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    const unsigned *w = c + 6 * gid;
    const int d = philox_draw31(w[0], w[1], w[2], w[3], w[4], w[5]);
    int d1, d2;
    philox_draw31_x2(w[0], w[1], w[2], w[3], w[4], w[5], d1, d2);
    out[gid] = make_uint4((unsigned)d, (unsigned)d1, (unsigned)d2, 0u);
}

// ---- section 2 ----
__global__ __launch_bounds__(PRIMS_THREADS) void masks_kernel(const int *__restrict__ recs, unsigned *__restrict__ out, const int *__restrict__ groups, const int maxMsg2) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int *G = groups + 8 * (gid >> 6);
    // (wave-uniform in the kernels, and said so here)
    const int t = __builtin_amdgcn_readfirstlane(G[0]), maxRar = __builtin_amdgcn_readfirstlane(G[1]);
    const bool front = __builtin_amdgcn_readfirstlane(G[2]) != 0;
    const int i0 = __builtin_amdgcn_readfirstlane(G[3]), acNow = __builtin_amdgcn_readfirstlane(G[4]), acPrev = __builtin_amdgcn_readfirstlane(G[5]);
    const int nUE = __builtin_amdgcn_readfirstlane(G[6]);
    const PrimRec r = prims_record(recs + 4 * gid, t, maxRar, maxMsg2);
    const unsigned rarlim = (unsigned)(maxRar - 1) << PK_RAR_SHIFT; // as prach_cluster.hip / prach_lcluster.hip state it
    const int i = i0 + lane;
    const PassMasks A = pass_masks<false>(r.pk, r.rx, r.rz, t, rarlim, front, i, acNow, acPrev, nUE);
    const PassMasks B = pass_masks<true>(r.pk, r.rx, r.rz, t, rarlim, front, i, acNow, acPrev, nUE);
    const bool lc = light_case(r.pk, r.rx, r.rz, t, rarlim);
    auto bit = [&](const unsigned long long m) { return (unsigned)((m >> lane) & 1ull); };
    out[gid] = bit(A.light) | bit(A.quiet) << 1 | bit(A.done) << 2 | bit(A.trig) << 3 | bit(B.light) << 4 | bit(B.quiet) << 5 | bit(B.done) << 6 | bit(B.trig) << 7 |
               (lc ? 256u : 0u);
}

// caller tables without memory: any value will do for the properties the tests assert
struct PrimsTab {
    PRACH_HD int fcall(const int q) const { return (q & 1) ? INT_MAX : 500 + q; }
    PRACH_HD int lcall(const int p) const { return (p & 2) ? 2000 + p : 3; }
};
// the branched body on one record at the start of subframe t (the reference of section 2)
void masks_host_record(const PrimRec r, const int t, const int maxRar, const int maxMsg2, const int i, const unsigned salt, unsigned *o) {
    const int tb0 = t - PRIMS_TB_BACK;
    UeState u = unpack(make_int4(r.rx, tb0, r.rz, (int)r.pk));
    if (u.pend == PEND_STAY) u.rar += t - 1 - r.rx; // written at subframe rx, not touched since: rarWindow has grown by the record's age
    UeK K;
    K.maxRar = maxRar; K.maxMsg2 = maxMsg2; K.aT = 5; K.withnoma = true;
    K.fmP = make_fastmod(54); K.fmB = make_fastmod(20); K.fmA = make_fastmod(5); K.fm5 = make_fastmod(5);
    const bool applied = ue_apply(u, (r.pk & PK_GRANT_BIT) != 0u, i, t - 1, K.fmA, PrimsTab{});
    const UePlan pl = ue_plan(u, t, maxRar, maxMsg2);
    ColdRegs cold{0x11111111, 0x22222222, 0x33333333, 0x44444444};
    int c_succ = 0x5555, c_contf = 0x6666;
    const int d1 = (int)((salt * 2654435761u) >> 1), d2 = (int)((salt * 40503u + 12345u) & 0x7fffffffu);
    const UeOut uo = ue_select(u, pl, d1, d2, i, t, t % 5, K, cold, c_succ, c_contf);
    const bool coldt = cold.ptc != 0x11111111 || cold.ftt != 0x22222222 || cold.stt != 0x33333333 || cold.fcnt != 0x44444444;
    const bool cnt = c_succ != 0x5555 || c_contf != 0x6666;
    const int4 p = pack(u);
    o[0] = (applied ? 1u : 0u) | (uo.dirty ? 2u : 0u) | ((unsigned)pl.need << 2) | ((unsigned)uo.evtype << 4) | (coldt ? 128u : 0u) | (cnt ? 256u : 0u);
    o[1] = (unsigned)p.x; o[2] = (unsigned)p.z; o[3] = (unsigned)p.w; o[4] = (unsigned)r.rx; o[5] = (unsigned)r.rz; o[6] = r.pk; o[7] = (unsigned)p.y;
}

// ---- section 3 ----
__global__ __launch_bounds__(PRIMS_THREADS) void wave_kernel(const int *__restrict__ rows, int4 *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    const int x = rows[gid];
    out[gid] = make_int4(wave_scan_incl(x), wave_sum(x), wave_max(x), 0);
}

// ---- section 4 ----
struct ModOut { unsigned w[8]; };
PRACH_HD ModOut mod_case(const int *c) {
    const FastMod f = make_fastmod(c[1]), fa = make_fastmod(c[3]);
    ModOut o;
    o.w[0] = (unsigned)fastmod(c[0], f); o.w[1] = (unsigned)fastmod_flat(c[0], f);
    o.w[2] = (unsigned)slot_align_fm(c[2], fa); o.w[3] = (unsigned)slot_align_flat(c[2], fa); o.w[4] = (unsigned)slot_align(c[2], c[3]);
    o.w[5] = f.M; o.w[6] = 0u; o.w[7] = 0u;
    return o;
}
__global__ __launch_bounds__(PRIMS_THREADS) void mod_kernel(const int *__restrict__ c, ModOut *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    out[gid] = mod_case(c + 4 * gid);
}

// ---- section 5 ----
__global__ __launch_bounds__(PRIMS_THREADS) void sector_kernel(const int *__restrict__ d, unsigned *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    out[gid] = (unsigned)sector_of_draw(d[gid]);
}

// ---- section 6 ----
__global__ __launch_bounds__(PRIMS_THREADS) void granule_kernel(const unsigned *__restrict__ c, uint4 *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    const unsigned *w = c + 5 * gid;
    const long long made = mk_granule(w[1], w[2], w[3]), raw = (long long)(((unsigned long long)w[2] << 32) | w[1]);
    const long long g = w[0] == 0u ? made : raw;
    out[gid] = make_uint4((unsigned)g, (unsigned)((unsigned long long)g >> 32), granule_ok(g, w[3]) ? 1u : 0u, granule_ok(g, w[4]) ? 1u : 0u);
}

// ---- section 7 ----
__global__ __launch_bounds__(64) void blocks_kernel(const int G, const int xpack, const int ntrials, unsigned *__restrict__ out) {
    int T = -1, b = -1;
    const bool ok = cluster_block(G, xpack, ntrials, T, b);
    const bool fits = T >= 0 && T < (1 << 20) && b >= 0 && b < 256;
    out[(size_t)blockIdx.x * 64 + threadIdx.x] = (ok ? 0x80000000u : 0u) | (fits ? 0x40000000u : 0u) | (((unsigned)T & 0xFFFFFu) << 8) | ((unsigned)b & 0xFFu);
}

// ---- section 8 ----
struct HotOut { int w[8]; };
__global__ __launch_bounds__(PRIMS_THREADS) void hot_kernel(const int *__restrict__ c, HotOut *__restrict__ out) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    const int *w = c + 3 * gid;
    const v2i_t h = hot_encode(w[0], w[1], w[2]);
    const int4 r = hot_decode(h, 0x7b7b7b7b);
    HotOut o;
    o.w[0] = h.x; o.w[1] = h.y; o.w[2] = r.x; o.w[3] = r.z; o.w[4] = r.w; o.w[5] = r.y; o.w[6] = hot_fits(w[0], w[1]) ? 1 : 0; o.w[7] = 0;
    out[gid] = o;
}
__global__ __launch_bounds__(PRIMS_THREADS) void slots_kernel(const int *__restrict__ pairs, int2 *__restrict__ out, const int lslots) {
    const size_t gid = (size_t)blockIdx.x * PRIMS_THREADS + threadIdx.x;
    const int *p = pairs + 2 * (gid / (size_t)lslots);
    CtxT<REC_L16> C;
    memset(&C, 0, sizeof C);
    C.G = p[0]; C.b = p[1]; C.fmG = make_fastmod(p[0]); // as cluster_kernel sets it up
    const int slot = (int)(gid % (size_t)lslots);
    const int idx = idx_of(C, slot);
    out[gid] = make_int2(idx, slot_of(C, idx));
}

#define CHK(call)                                                                                            \
    do {                                                                                                     \
        const hipError_t rc_ = (call);                                                                       \
        if (rc_ != hipSuccess) {                                                                             \
            fprintf(stderr, "gpu_prims_harness: %s: %s (line %d)\n", #call, hipGetErrorString(rc_), __LINE__); \
            return 2;                                                                                        \
        }                                                                                                    \
    } while (0)

int fail(const char *what) {
    fprintf(stderr, "gpu_prims_harness: %s\n", what);
    return 3;
}

int write_result(const char *path, const int section, const int host, const int n, const std::vector<unsigned> &body) {
    const unsigned head[4] = {(unsigned)PRIMS_MAGIC, (unsigned)section, (unsigned)host, (unsigned)n};
    FILE *g = fopen(path, "wb");
    if (!g) return fail("cannot open the result file");
    size_t put = fwrite(head, 4, 4, g);
    if (!body.empty()) put += fwrite(body.data(), 4, body.size(), g);
    if (fclose(g) != 0 || put != 4 + body.size()) return fail("result file: short write");
    return 0;
}

size_t padded(const size_t n, const size_t unit) { return (n + unit - 1) / unit * unit; }

// `n` cases of `wpc` words each, padded to `npad` cases with copies of the first one
std::vector<int> pad_cases(const int *src, const size_t n, const size_t wpc, const size_t npad) {
    std::vector<int> v(npad * wpc);
    memcpy(v.data(), src, 4 * n * wpc);
    for (size_t k = n; k < npad; k++) memcpy(v.data() + k * wpc, src, 4 * wpc);
    return v;
}

// One launch of a kernel(in, out) over npad threads: `inw` words in, `outw` words out per thread; the first n threads' output is kept.
template <class IN, class OUT, class... X>
int run_simple(void (*kernel)(const IN *, OUT *, X...), const std::vector<int> &in, const size_t n, const size_t npad, const size_t outw, std::vector<unsigned> &body,
               X... extra) {
    if (npad % PRIMS_THREADS || npad == 0 || npad > PRIMS_MAX_THREADS) return fail("thread count out of range");
    int *din = nullptr;
    unsigned *dout = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&din), 4 * in.size()));
    CHK(hipMalloc(reinterpret_cast<void **>(&dout), 4 * npad * outw));
    CHK(hipMemcpy(din, in.data(), 4 * in.size(), hipMemcpyHostToDevice));
    CHK(hipMemset(dout, 0xA5, 4 * npad * outw));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(npad / PRIMS_THREADS)), dim3(PRIMS_THREADS), 0, nullptr, reinterpret_cast<const IN *>(din), reinterpret_cast<OUT *>(dout), extra...);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    const size_t at = body.size();
    body.resize(at + n * outw);
    CHK(hipMemcpy(body.data() + at, dout, 4 * n * outw, hipMemcpyDeviceToHost));
    CHK(hipFree(din));
    CHK(hipFree(dout));
    return 0;
}

// ---- validation: lengths and every index a kernel will form ----
struct Case {
    std::vector<int> w;
    int section, n, p3, p4;
    const int *payload() const { return w.data() + 16; }
    size_t words() const { return w.size() - 16; }
};

int check_masks(const Case &c) {
    if (c.n % 64 || c.words() != (size_t)c.n / 64 * 8 + (size_t)c.n * 4) return fail("masks: file length");
    if (c.p3 < 0 || c.p3 > 254) return fail("masks: maxMsg2 out of range");
    const int *groups = c.payload(), *recs = groups + (size_t)c.n / 64 * 8;
    for (int g = 0; g < c.n / 64; g++) {
        const int *G = groups + 8 * (size_t)g;
        if (G[0] < 8 || G[0] > 65000 || G[1] < 1 || G[1] > 200 || (G[2] != 0 && G[2] != 1)) return fail("masks: group parameters out of range");
        if (G[3] < 0 || G[3] > (1 << 24) || G[3] % 64 || G[4] < 0 || G[5] < 0 || G[6] < 0) return fail("masks: group range out of range");
        for (int l = 0; l < 64; l++) {
            const int *r = recs + 4 * ((size_t)g * 64 + l);
            if (r[0] != 0 && r[0] != 1) return fail("masks: record kind");
            if (r[0] == 0 && (unsigned)r[1] >= prims_enum_size(G[1])) return fail("masks: enumeration index out of range");
        }
    }
    return 0;
}

int check_mod(const Case &c) {
    if (c.words() != (size_t)c.n * 4) return fail("mod: file length");
    for (int k = 0; k < c.n; k++) {
        const int *m = c.payload() + 4 * (size_t)k;
        if (m[1] < 1 || m[3] < 1 || m[3] > 20 || m[2] < 0 || m[2] > INT_MAX - 32) return fail("mod: divisor / subframe out of range");
    }
    return 0;
}

int read_case(const char *path, Case &c) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail("cannot open the case file");
    fseek(f, 0, SEEK_END);
    const long fbytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (fbytes < 64 || fbytes % 4) { fclose(f); return fail("case file: bad length"); }
    c.w.resize((size_t)fbytes / 4);
    const size_t got = fread(c.w.data(), 4, c.w.size(), f);
    fclose(f);
    if (got != c.w.size()) return fail("case file: short read");
    c.section = c.w[1]; c.n = c.w[2]; c.p3 = c.w[3]; c.p4 = c.w[4];
    if (c.w[0] != PRIMS_MAGIC || c.section < 1 || c.section > 9 || c.n < 1 || (size_t)c.n > PRIMS_MAX_THREADS) return fail("case file: bad header");
    return 0;
}

int run_blocks(const Case &c, std::vector<unsigned> &body) {
    if (c.words() != 4 * (size_t)c.n) return fail("blocks: file length");
    size_t total = 0;
    for (int k = 0; k < c.n; k++) {
        const int *s = c.payload() + 4 * (size_t)k;
        if (s[0] < 1 || s[0] > 64 || (s[1] != 0 && s[1] != 1) || s[2] < 1 || s[2] > 4096 || s[3] < 1 || s[3] > PRIMS_MAX_GRID7) return fail("blocks: parameters out of range");
        total += (size_t)s[3] * 64;
    }
    if (total > 4 * PRIMS_MAX_THREADS) return fail("blocks: too many threads");
    unsigned *dout = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&dout), 4 * total));
    CHK(hipMemset(dout, 0xA5, 4 * total));
    size_t at = 0;
    for (int k = 0; k < c.n; k++) { // one launch per set: cluster_block reads the launch's own blockIdx
        const int *s = c.payload() + 4 * (size_t)k;
        hipLaunchKernelGGL(blocks_kernel, dim3((unsigned)s[3]), dim3(64), 0, nullptr, s[0], s[1], s[2], dout + at);
        CHK(hipGetLastError());
        at += (size_t)s[3] * 64;
    }
    CHK(hipDeviceSynchronize());
    body.resize(total);
    CHK(hipMemcpy(body.data(), dout, 4 * total, hipMemcpyDeviceToHost));
    return 0;
}

int run_hot(const Case &c, std::vector<unsigned> &body) {
    const size_t n = (size_t)c.n;
    if (c.p3 < 1 || c.p3 > 4096 || c.p4 < 64 || c.p4 > CLUSTER_LQCAP || c.p4 % 64 || c.words() != 3 * n + 2 * (size_t)c.p3) return fail("hot: file length");
    const int *pairs = c.payload() + 3 * n;
    for (int k = 0; k < c.p3; k++)
        if (pairs[2 * k] < 1 || pairs[2 * k] > CLUSTER_MAX_G || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= pairs[2 * k]) return fail("hot: (G, b) out of range");
    const size_t npad = padded(n, PRIMS_THREADS);
    int rc = run_simple<int, HotOut>(hot_kernel, pad_cases(c.payload(), n, 3, npad), n, npad, 8, body);
    if (rc) return rc;
    const size_t ns = (size_t)c.p3 * (size_t)c.p4; // (lslots is a multiple of 64: whole wavefronts; pairs padded to whole workgroups)
    const size_t nspad = padded(ns, PRIMS_THREADS), ppad = (nspad + (size_t)c.p4 - 1) / (size_t)c.p4;
    return run_simple<int, int2, int>(slots_kernel, pad_cases(pairs, (size_t)c.p3, 2, ppad), ns, nspad, 2, body, c.p4);
}

int run_device(const Case &c, const char *res_path) {
    const size_t n = (size_t)c.n;
    const size_t npad = padded(n, PRIMS_THREADS);
    std::vector<unsigned> body;
    int rc = 0;
    switch (c.section) {
    case 1:
        if (c.words() != 6 * n || c.n > 20000) return fail("philox: file length");
        rc = run_simple<unsigned, uint4>(philox_kernel, pad_cases(c.payload(), n, 6, npad), n, npad, 4, body);
        break;
    case 2: {
        if ((rc = check_masks(c)) != 0) return rc;
        const size_t ng = n / 64;
        const std::vector<int> groups = pad_cases(c.payload(), ng, 8, npad / 64); // (padding wavefronts: the first group's parameters with the first record)
        int *dg = nullptr;
        CHK(hipMalloc(reinterpret_cast<void **>(&dg), 4 * groups.size()));
        CHK(hipMemcpy(dg, groups.data(), 4 * groups.size(), hipMemcpyHostToDevice));
        rc = run_simple<int, unsigned, const int *, int>(masks_kernel, pad_cases(c.payload() + ng * 8, n, 4, npad), n, npad, 1, body, dg, c.p3);
        break;
    }
    case 3:
        if (c.words() != 64 * n) return fail("wave: file length");
        rc = run_simple<int, int4>(wave_kernel, pad_cases(c.payload(), n, 64, padded(n, 4)), n * 64, padded(n, 4) * 64, 4, body);
        break;
    case 4:
        if ((rc = check_mod(c)) != 0) return rc;
        rc = run_simple<int, ModOut>(mod_kernel, pad_cases(c.payload(), n, 4, npad), n, npad, 8, body);
        break;
    case 5:
        if (c.words() != n) return fail("sector: file length");
        for (size_t k = 0; k < n; k++) if (c.payload()[k] < 0) return fail("sector: a draw is never negative");
        rc = run_simple<int, unsigned>(sector_kernel, pad_cases(c.payload(), n, 1, npad), n, npad, 1, body);
        break;
    case 6:
        if (c.words() != 5 * n) return fail("granule: file length");
        for (size_t k = 0; k < n; k++) if (c.payload()[5 * k] != 0 && c.payload()[5 * k] != 1) return fail("granule: case kind");
        rc = run_simple<unsigned, uint4>(granule_kernel, pad_cases(c.payload(), n, 5, npad), n, npad, 4, body);
        break;
    case 7: rc = run_blocks(c, body); break;
    case 8: rc = run_hot(c, body); break;
    default: return fail("section has no device part");
    }
    if (rc) return rc;
    return write_result(res_path, c.section, 0, c.n, body);
}

int run_host(const Case &c, const char *res_path) {
    const size_t n = (size_t)c.n;
    std::vector<unsigned> body;
    int rc = 0;
    if (c.section == 2) {
        if ((rc = check_masks(c)) != 0) return rc;
        const int *groups = c.payload(), *recs = groups + n / 64 * 8;
        body.resize(8 * n);
        for (size_t k = 0; k < n; k++) {
            const int *G = groups + 8 * (k >> 6);
            masks_host_record(prims_record(recs + 4 * k, G[0], G[1], c.p3), G[0], G[1], c.p3, G[3] + (int)(k & 63), (unsigned)k, body.data() + 8 * k);
        }
    } else if (c.section == 4) {
        if ((rc = check_mod(c)) != 0) return rc;
        body.resize(8 * n);
        for (size_t k = 0; k < n; k++) { const ModOut o = mod_case(c.payload() + 4 * k); memcpy(body.data() + 8 * k, o.w, 32); }
    } else if (c.section == 9) {
        if (c.words() != 4 * n) return fail("pack: file length");
        body.resize(13 * n);
        for (size_t k = 0; k < n; k++) {
            const int *r = c.payload() + 4 * k;
            const UeState u = unpack(make_int4(r[0], r[1], r[2], r[3]));
            const int4 p = pack(u);
            const int o[13] = {u.tx, u.tb, u.bo, u.act, u.conn, u.pre, u.rar, u.mrc, u.pend, p.w, p.x, p.y, p.z};
            memcpy(body.data() + 13 * k, o, sizeof o);
        }
    } else {
        return fail("section has no host part");
    }
    return write_result(res_path, c.section, 1, c.n, body);
}

} // namespace
} // namespace prach

int main(int argc, char **argv) {
    using namespace prach;
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("PK_ACT_SHIFT %u\nPK_CONN_SHIFT %u\nPK_PRE_SHIFT %u\nPK_RAR_SHIFT %u\nPK_MRC_SHIFT %u\nPK_PEND_SHIFT %u\nPK_GRANT_BIT %u\n", PK_ACT_SHIFT, PK_CONN_SHIFT,
               PK_PRE_SHIFT, PK_RAR_SHIFT, PK_MRC_SHIFT, PK_PEND_SHIFT, PK_GRANT_BIT);
        printf("ACT_IDLE %d\nACT_DONE %d\nACT_M1 %d\nACT_M3 %d\nPEND_NONE %d\nPEND_STAY %d\nPEND_CALLER %d\nPEND_RESET %d\nPEND_PASSIVE %d\nPEND_RJOIN %d\n", ACT_IDLE, ACT_DONE,
               ACT_M1, ACT_M3, PEND_NONE, PEND_STAY, PEND_CALLER, PEND_RESET, PEND_PASSIVE, PEND_RJOIN);
        printf("HOT_BO_BIAS %d\nGR_NONE %u\nSPIN_LIMIT %u\nUEV_NONE %d\nUEV_CALLER %d\nUEV_RESETCAND %d\nUEV_RJOIN %d\n", HOT_BO_BIAS, GR_NONE, SPIN_LIMIT, UEV_NONE, UEV_CALLER,
               UEV_RESETCAND, UEV_RJOIN);
        printf("CLUSTER_LQCAP %d\nCLUSTER_MAX_G %d\nPRIMS_TB_BACK %d\nPRIMS_THREADS %d\n", CLUSTER_LQCAP, CLUSTER_MAX_G, PRIMS_TB_BACK, PRIMS_THREADS);
        return 0;
    }
    const bool host = argc == 5 && !strcmp(argv[1], "--host");
    if (!host && argc != 4) return fail("usage: gpu_prims_harness [--host] SECTION CASE RESULT | --constants");
    char **a = argv + (host ? 2 : 1);
    Case c;
    const int rc = read_case(a[1], c);
    if (rc) return rc;
    if (atoi(a[0]) != c.section) return fail("the case file belongs to another section");
    return host ? run_host(c, a[2]) : run_device(c, a[2]);
}
