// prach_engine.hip — host side of libprach_hip.so: the engine behind the C ABI in include/prach.h.
// Owns the HIP stream, one device arena and one pinned staging buffer (both grown on demand, nothing is
// allocated per subframe or per trial), stages the per-trial parameter blocks / arrival tables / draw-stream
// seeds of a whole launch with ONE copy, launches the trial kernels and turns DevResult into prach_result.
// There is NO CPU fallback: without a gfx950 device every entry point that simulates returns PRACH_ERR_DEVICE.
#include "prach_device.h"
#include "prach_grouped.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits.h>
#include <new>
#include <thread>
#include <vector>

using namespace prach;

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            std::fprintf(stderr, "[prach] HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, \
                         __LINE__, hipGetErrorString(e_));                                            \
            return PRACH_ERR_DEVICE;                                                                  \
        }                                                                                             \
    } while (0)

struct prach_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    char *arena = nullptr;
    size_t arena_cap = 0;
    // the arena as ONE reserved virtual range that physical memory is mapped into piece by piece (hipMemAddressReserve / hipMemCreate / hipMemMap): growing it
    // maps the increment only — no hipFree + hipMalloc of the whole arena (measured 0.8-1.4 s for 10-16 GB when a sweep's calls grow point by point) — and
    // its address never changes.  vmm: 0 untried, 1 in use, -1 unavailable (plain hipMalloc arena).
    int vmm = 0;
    size_t vmm_reserved = 0, vmm_gran = 0;
    std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> vmm_parts;
    char *pinned = nullptr; // host staging mirror of the head of the arena (parameter blocks, arrival tables, stream seeds, results)
    size_t pinned_cap = 0;
    // The device reduction of a call (prach_run_trials_dist, _timeline, _sojourn, _summary or _trace: a call runs at most one, so all kinds share these): the call's
    // counters (zeroed once per call, copied out once at its end — not part of the arena, which is laid out again for every launch), the job table of one
    // launch, pinned and on the device, in bytes (DistJob, TimelineJob or TraceJob elements), and the events around the reduction kernel of a launch
    // (prach_timing.dist_ms / timeline_ms / sojourn_ms).  All created and grown at the start of a call, never per launch.
    char *red_buf = nullptr;
    size_t red_cap = 0;
    char *red_jobs_h = nullptr, *red_jobs_d = nullptr;
    size_t red_jobs_cap = 0;
    hipEvent_t red_ev0 = nullptr, red_ev1 = nullptr;
    // ... and, where the kind has them (Reduction): the bulk part the kernel writes with plain stores — the engine's own buffer (bulk_buf, grown at the start
    // of a call) or device memory of the caller's — with the bytes from one of its rows to the next, and the call's table behind the counters in red_buf
    char *bulk_buf = nullptr;
    size_t bulk_cap = 0;
    char *red_bulk = nullptr;
    size_t red_bulk_pitch = 0;
    const char *red_table = nullptr;
    int64_t opt_trace_scheme = 1;    // trace_kernel's binning (prach_trace.hip): 0 global atomics only, 1 the tile's bins added up in an LDS window first
    int64_t opt_summary_threads = 1024; // summary_kernel's workgroup (prach_summary.hip): 512 or 1024 threads, one workgroup per trial
    int64_t opt_pick_threads = 1024;    // pick_kernel's workgroup (prach_pick.hip): 512 or 1024 threads, one workgroup per trial
    int64_t opt_xtab_scheme = 1;     // xtab_kernel's binning (prach_xtab.hip): 0 global atomics only, 1 a table that fits privatised in LDS
    int64_t opt_sojourn_scheme = 1;  // sojourn_kernel's binning (prach_sojourn.hip): 0 global atomics only, 1 rows of the histogram privatised in LDS
    int64_t opt_noma_timeline_window = NTL_WINDOW; // noma_timeline_kernel's LDS window in bins (prach_noma_timeline.hip; measured: profiles/noma_timeline_kernel.md)
    int64_t opt_timeline_scheme = 1; // timeline_kernel's binning (prach_timeline.hip): 0 global atomics only, 1 windows of bins privatised in LDS (measured faster: DESIGN.md 4)
    int64_t opt_dist_scheme = 1;   // dist_kernel's binning of the preamble counts (prach_dist.hip): 0 plain LDS adds, 1 per-wavefront copies (measured fastest), 2 match and aggregate
    prach_timing last{};
    int64_t opt_stream_factor = 0; // glibc: initial draws-per-UE budget override (0 = auto)
    double draws_per_ue_seen = 0;  // glibc: the largest rand() consumption per UE of the last call's trials (0: none yet) — sizes the next call's stream windows
    int64_t opt_cluster = 0;       // workgroups per trial for the Philox cluster kernel (0 = auto)
    int64_t opt_legacy = 0;        // 1: run Philox trials on the one-workgroup trial_kernel as well
    int64_t opt_dense = 0;         // 1: cluster kernel without the compacted pass (diagnostic)
    int64_t opt_wide_records = 0;  // 1: 16-byte records also with one workgroup per trial (diagnostic)
    int64_t opt_pipeline = 1;      // 0: clusters do not run phase A ahead of the exchange (diagnostic)
    int64_t opt_resident = 0;      // test hook: pretend only this many workgroups can be co-resident (0 = ask the runtime)
    int64_t opt_host_threads = 0;  // host threads for the NOMA.c activation tables (0 = all cores)
#ifdef PRACH_QCAP                  // (the small-queue test build exists to exercise the queue-overflow path of the global-record kernels)
    int64_t opt_lds_records = 0;
#else
    int64_t opt_lds_records = 1;   // 0: clusters keep their UE records in global memory (diagnostic)
#endif
    int64_t opt_xcd_pack = 1;      // 1: lean clusters are launched XCD-packed (a cluster per XCD; granules stay in that XCD's L2 once verified)
    int64_t opt_fast = 1;          // 0: LDS-resident clusters run on the general kernel (prach_cluster.hip) instead of prach_lcluster.hip
    int64_t opt_batch_waves = 0;   // wavefronts per batch-kernel workgroup: 8 (512 threads, two trials per CU), 16 (one), 0 = chosen per launch
    int64_t opt_plain_arena = 0;   // 1: the arena is one hipMalloc allocation, re-allocated when it grows (diagnostic)
    int64_t opt_vmm_fail_after = 0; // test hook: the reserved-range arena cannot map a further piece once it has this many (0: no limit)
    int64_t opt_noma_host_activation = 0; // 1: NOMA.c's activeUE table is built on the host (the reference's libm) instead of by noma_activation_kernel
    int64_t opt_noma_ambiguity_test = 0;  // test hook: the resolver reports every gain sort as ambiguous (exercises the rerun with the host-built table)
    int64_t opt_calendar_cap = 0;  // test hook: entries per calendar list of the batch kernel (0 = sized per trial)
    int num_cus = 256;
    size_t mem_budget = (size_t)200 << 30; // arena bytes one launch may take (3/4 of the device's memory): a call that needs more runs as several launches
};

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct TrialLayout {
    size_t rec, ptc, ftt, stt, fcnt, nd, evbuf, evbuf2, sidx, sched, stream, logs, timers, out, mbox, cand;
    size_t trace; // prach_run_trials_trace: one 16-byte row per subframe, in the zeroed region (0: none)
    size_t n_pre0, n_sector, n_gain, n_lgain, n_nd0, sector;
    size_t n_level, gain_edges; // prach_run_trials_noma_gain: the trial's 4-byte-per-UE level column; the launch's list of EDGE UEs (in the zeroed region, the same in every trial; 0: none)
    size_t rec32, chunks, ctab, cpool, jcal, qov, evov; // batch kernel
    int calcap, calslots, npool, tcap;
    size_t diag;                 // diagnostic build: per-workgroup stamps (zeroed region)
    size_t seeds, nchunks; // glibc: one 31-word window per STREAM_CHUNK outputs (device-side generation)
    size_t stream_len, sched_len;
    int evw, mbstride;
};

// Arena of one launch:
//   [ TrialDev[m] | arrival tables | glibc stream seeds ]   staged region: built in pinned host memory, ONE copy
//   [ DevResult[m] | mailboxes ]                             zeroed region: ONE memset per launch (tags: 0 never equals t+1);
//                                                            the DevResult block also comes back with ONE copy
//   [ per-trial arrays ]                                     records, cold fields, scratch of the kernel that runs
struct LaunchLayout {
    std::vector<TrialLayout> t;
    size_t staged_end = 0, zero_begin = 0, zero_end = 0, out0 = 0, end = 0;
    size_t act_flags = 0; // NOMA.c: noma_activation_kernel's list of UEs for the host (in the zeroed region)
    size_t stream_jobs = 0; // glibc: StreamJob[m] (in the staged region)
};

size_t mbox_bytes(const prach_cfg &c, int G, int &evw, int &mbstride) {
    evw = 0; mbstride = 0;
    if (G <= 0) return 0;
    const size_t n = (size_t)c.nUE;
    evw = G == 1 ? 4096 : CLUSTER_EVW;
    const size_t lgroups = ((n + 63) / 64 + (size_t)G - 1) / (size_t)G;
    mbstride = (int)align_up((size_t)2 * (1 + c.nPreamble + evw + (lgroups + 1) / 2), 4); // 8-byte granules: header, buckets, events, (glibc) group draw counts
    if (c.variant == PRACH_VARIANT_NOMA_C) mbstride = (int)align_up((size_t)2 * (1 + 6 * c.nPreamble), 4); // header + 6 x nP bins
    if (G == 1) return 256; // one workgroup per trial exchanges nothing
    return 4 * (size_t)2 * G * mbstride;
}

// stream_len[k]: glibc draw-stream window of trial k (0 in Philox mode); G: workgroups per trial (0 = trial_kernel)
// all_logs: every trial gets a device log region (the call's reduction reads it there: prach_run_trials_timeline, prach_run_trials_sojourn), not only the ones whose log the host asked for
// trace: every trial gets its per-subframe rows (prach_run_trials_trace): 16 bytes x maxTime, zeroed with the rest of the zeroed region
// levels: every NOMA.c trial gets a level column and the launch a list of EDGE UEs (prach_run_trials_noma_gain)
LaunchLayout layout_launch(const prach_cfg *cfgs, const int *idx, int m, prach_ue_log *const *ue_logs, bool all_logs, bool trace, bool levels, const std::vector<size_t> &stream_len, int G, bool batch, bool full_calendars, int64_t calendar_cap) {
    LaunchLayout L;
    L.t.resize(m);
    size_t o = align_up(sizeof(TrialDev) * (size_t)m, 256);
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    for (int k = 0; k < m; k++) { // staged region
        const prach_cfg &c = cfgs[idx[k]];
        TrialLayout &T = L.t[k];
        T.sched_len = (size_t)(prach_max_time(&c) / c.accessTime + 2);
        T.sched = take(4 * T.sched_len);
        T.stream_len = stream_len[k];
        T.nchunks = (T.stream_len + STREAM_CHUNK - 1) / STREAM_CHUNK;
        T.seeds = T.stream_len ? take(4 * 31 * (T.nchunks + 1)) : 0;
    }
    bool any_stream = false;
    for (int k = 0; k < m; k++) any_stream = any_stream || stream_len[k] > 0;
    if (any_stream) L.stream_jobs = take(sizeof(StreamJob) * (size_t)m);
    L.staged_end = o;
    L.zero_begin = o;
    L.out0 = take(sizeof(DevResult) * (size_t)m);
    for (int k = 0; k < m; k++) {
        L.t[k].out = L.out0 + sizeof(DevResult) * (size_t)k;
        const size_t mb = mbox_bytes(cfgs[idx[k]], G, L.t[k].evw, L.t[k].mbstride);
        L.t[k].mbox = mb ? take(mb) : 0;
#ifdef PRACH_STAMPS
        L.t[k].diag = G > 1 ? take(8 * 32 * (size_t)CLUSTER_MAX_G) : 0;
#else
        L.t[k].diag = 0;
#endif
        { // (NOMA.c, prach_run_trials_noma_trace: 32 bytes per access slot and sector)
            const prach_cfg &c = cfgs[idx[k]];
            const size_t mt = (size_t)prach_max_time(&c);
            L.t[k].trace = !trace ? 0 : c.variant == PRACH_VARIANT_NOMA_C ? take(32 * 6 * ((mt + (size_t)c.accessTime - 1) / (size_t)c.accessTime)) : take(16 * mt);
        }
    }
    if (cfgs[idx[0]].variant == PRACH_VARIANT_NOMA_C) L.act_flags = take(4 * (2 + 2 * (size_t)NOMA_ACT_FLAG_CAP));
    const size_t gain_edges = levels ? take(4 * (2 + 2 * (size_t)NG_EDGE_CAP)) : 0;
    L.zero_end = o;
    for (int k = 0; k < m; k++) {
        const prach_cfg &c = cfgs[idx[k]];
        TrialLayout &T = L.t[k];
        const size_t n = (size_t)c.nUE;
        T.rec = T.ptc = T.ftt = T.stt = T.fcnt = T.nd = T.rec32 = T.chunks = T.ctab = T.cpool = T.jcal = T.qov = T.evov = 0;
        T.calcap = T.calslots = T.npool = T.tcap = 0;
        if (batch) { // prach_batch.hip: 32-byte event records, the two calendars, the global parts of the candidate and event lists
            // The records of the UEs under way travel in 2 KB chunks of 64: every UE has one record, so ceil(nUE / 64) full chunks, plus the open chunks of the
            // wavefronts (at most 128 each), plus what sits in their stacks of free ids (64 each), plus slack: twice the full chunks + 3 136.  A join list holds
            // the UEs whose window opens in ONE subframe: txTime is aligned to the access slots (Beta.c:268-277), so an overloaded trial (more UEs than its UL
            // grants can serve: every UE cycles through backoff and window about every 17 subframes) puts ~0.3 nUE into one list, another trial far less.
            // A trial that exhausts either leaves with PRACH_ERR_INTERNAL and is rerun with a doubled pool and lists of nUE entries (run_trials_impl).
            T.calslots = batch_calendar_slots(c.backoff, c.accessTime, c.maxRarWindow);
            const double steps_ = (double)((c.max_steps > 0 && c.max_steps < prach_max_time(&c)) ? c.max_steps : prach_max_time(&c));
            const bool overloaded = (double)c.nUE > (double)std::max(0, c.nGrantUL - 1) * steps_ / 5.0;
            T.calcap = (int)(n <= 16384 ? n : std::max<size_t>(16384, overloaded ? n * 2 / 5 : n / 8)) + 64; // (a small trial gets lists that cannot fill)
            if (calendar_cap > 0) T.calcap = (int)calendar_cap;
            T.npool = 2 * (int)((n + 63) / 64) + 16 * (128 + 64) + 64;
            if (full_calendars) { T.calcap = (int)n + 64; T.npool *= 2; }
            T.tcap = (int)((n + 63) / 64) + 256;
            T.rec32 = take(32 * n); T.chunks = take((size_t)batch_chunk_bytes() * (size_t)T.npool); T.ctab = take(4 * (size_t)T.calslots * (size_t)T.tcap);
            T.cpool = take(8 * (size_t)T.npool); T.jcal = take(4 * ((size_t)T.calslots * (size_t)T.calcap + 64)); // (+ 64 words: where lanes without a join entry store, prach_batch.hip)
            T.qov = take(4 * n); T.evov = take(16 * n);
        } else {
            T.rec = take(16 * n);
            T.ptc = take(4 * n); T.ftt = take(4 * n); T.stt = take(4 * n); T.fcnt = take(4 * n); T.nd = take(4 * n);
        }
        T.evbuf = T.evbuf2 = T.sidx = T.cand = 0;
        if (G == 0) { // trial_kernel only: event / singleton scratch without a per-subframe capacity
            T.evbuf = take(sizeof(Event) * n); T.evbuf2 = take(sizeof(Event) * n);
            T.sidx = take(4 * (n + 256));
        } else if (c.variant != PRACH_VARIANT_NOMA_C) {
            T.cand = take(8 * (n + 64 * (size_t)G + 64)); // cluster kernel: early-leaver candidates
        }
        T.stream = T.stream_len ? take(4 * (T.stream_len + 2)) : 0;
        T.logs = (all_logs || (ue_logs && ue_logs[idx[k]])) ? take(sizeof(prach_ue_log) * n) : 0;
        T.timers = take(4 * n);
        T.sector = (c.flags & PRACH_FLAG_SECTOR_GRANTS) ? take(4 * n) : 0;
        T.n_pre0 = T.n_sector = T.n_gain = T.n_lgain = T.n_nd0 = 0;
        if (c.variant == PRACH_VARIANT_NOMA_C) {
            T.n_pre0 = take(4 * n); T.n_sector = take(4 * n); T.n_gain = take(8 * n); T.n_lgain = take(8 * n); T.n_nd0 = take(4 * n);
        }
        T.n_level = levels && c.variant == PRACH_VARIANT_NOMA_C ? take(4 * n) : 0;
        T.gain_edges = gain_edges;
    }
    L.end = o;
    return L;
}

// initial glibc stream budget (draws) for a trial; the kernel reports exhaustion and we retry bigger
// (a sweep is called point after point with growing nUE: what the previous point's trials consumed per UE, tripled, is the first window of the next —
//  a Beta.c point with 54 grants draws ~30 values per UE, not 450: 100 seeds x 100 000 UEs are then 3 GB of windows instead of 18 GB; a window that
//  turns out too small is the ordinary PRACH_ERR_STREAM retry, four times larger)
uint64_t stream_budget(const prach_cfg &c, int attempt, int64_t factor, double seen) {
    uint64_t per = factor > 0 ? (uint64_t)factor : seen > 0 ? (uint64_t)std::min(450.0, std::max(64.0, 3.0 * seen + 32.0)) : 450; // 100k UEs / 12 grants / backoff 20 consume ~325 per UE
    if (attempt > 0 && factor <= 0) per = 450; // (a window sized from a light previous call was too small: straight to the default, then four times larger per retry)
    uint64_t b = (uint64_t)c.nUE * per + (1u << 20);
    return b << (2 * std::max(0, attempt - (seen > 0 && factor <= 0 ? 1 : 0)));
}

// grows the reserved-range arena to at least `need` mapped bytes; false: the mechanism is not available here (nothing has been changed)
static bool grow_vmm_arena(prach_engine *e, size_t need) {
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = e->device;
    if (e->vmm == 0) {
        size_t gran = 0, free_b = 0, total_b = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || gran == 0) { (void)hipGetLastError(); e->vmm = -1; return false; }
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) { (void)hipGetLastError(); e->vmm = -1; return false; }
        const size_t reserve = align_up(total_b, gran); // (address space, not memory)
        void *p = nullptr;
        if (hipMemAddressReserve(&p, reserve, 0, nullptr, 0) != hipSuccess || !p) { (void)hipGetLastError(); e->vmm = -1; return false; }
        e->arena = static_cast<char *>(p); e->arena_cap = 0; e->vmm_reserved = reserve; e->vmm_gran = std::max(gran, (size_t)2 << 20); e->vmm = 1; // (pieces in multiples of 2 MB whatever the runtime recommends)
    }
    if (need > e->vmm_reserved) return false;
    // at least a quarter more than what is mapped, at least 256 MB: a sweep's growing calls map a handful of increments in all — each increment in pieces of
    // at most 1 GB (hipMemSetAccess refused pieces of 2 GB and more: hipErrorInvalidValue)
    size_t delta = align_up(std::max(need - e->arena_cap, std::max(e->arena_cap >> 2, (size_t)256 << 20)), e->vmm_gran);
    delta = std::min(delta, e->vmm_reserved - e->arena_cap);
    const size_t piece_max = align_up((size_t)1 << 30, e->vmm_gran); // (hipMemSetAccess refuses a piece of 2^31 bytes: hipErrorInvalidValue)
    while (delta > 0) {
        const size_t piece = std::min(delta, piece_max);
        if (e->opt_vmm_fail_after > 0 && (int64_t)e->vmm_parts.size() >= e->opt_vmm_fail_after) return false; // (test hook: as if the device had no more memory to map)
        hipMemGenericAllocationHandle_t h;
        auto why = [&](const char *what, hipError_t rc) { if (std::getenv("PRACH_VERBOSE")) std::fprintf(stderr, "[prach] %s of a %zu-byte piece at offset %zu: %s\n", what, piece, e->arena_cap, hipGetErrorName(rc)); (void)hipGetLastError(); };
        hipError_t rc = hipMemCreate(&h, piece, &prop, 0);
        if (rc != hipSuccess) { why("hipMemCreate", rc); return false; }
        rc = hipMemMap(e->arena + e->arena_cap, piece, 0, h, 0);
        if (rc != hipSuccess) { why("hipMemMap", rc); (void)hipMemRelease(h); return false; }
        hipMemAccessDesc acc{};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        // (access is set for the whole mapped range from the base: inside this engine the runtime refuses the new piece alone — hipErrorInvalidValue for every
        //  piece behind the first, of any size — although profiles/tools/vmm_probe.hip, the same calls in a bare program, is granted it)
        rc = hipMemSetAccess(e->arena, e->arena_cap + piece, &acc, 1);
        if (rc != hipSuccess) { why("hipMemSetAccess", rc); (void)hipMemUnmap(e->arena + e->arena_cap, piece); (void)hipMemRelease(h); return false; }
        e->vmm_parts.push_back({h, piece});
        e->arena_cap += piece; // (pieces mapped before a failure stay: the caller sees the arena short of `need` and falls back)
        delta -= piece;
    }
    return true;
}
static void free_arena(prach_engine *e) {
    if (e->vmm == 1) {
        size_t at = 0;
        for (auto &pt : e->vmm_parts) { (void)hipMemUnmap(e->arena + at, pt.second); (void)hipMemRelease(pt.first); at += pt.second; }
        e->vmm_parts.clear();
        if (e->arena) (void)hipMemAddressFree(e->arena, e->vmm_reserved);
    } else if (e->arena) (void)hipFree(e->arena);
    e->arena = nullptr; e->arena_cap = 0;
}

int ensure_arena(prach_engine *e, size_t need) {
    if (need <= e->arena_cap) return PRACH_OK;
    if (e->vmm >= 0 && !e->opt_plain_arena) {
        if (grow_vmm_arena(e, need) && need <= e->arena_cap) return PRACH_OK;
        if (e->vmm == 1) { // the range is in use but could not grow (out of memory / of range): back to one plain allocation
            std::fprintf(stderr, "[prach] the reserved-range arena could not grow to %zu bytes: falling back to hipMalloc\n", need);
            free_arena(e);
        }
        e->vmm = -1;
    }
    const size_t had = e->arena_cap;
    if (e->arena) HIPCHK(hipFree(e->arena));
    e->arena = nullptr;
    e->arena_cap = 0;
    // (a sweep's calls grow point by point: growing by an eighth re-allocated at nearly every point, and one hipFree + hipMalloc of ~16 GB measured 1.4 s)
    const size_t want = std::max(need + (need >> 2), std::min<size_t>(2 * had, (size_t)64 << 30));
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&e->arena), want));
    e->arena_cap = want;
    return PRACH_OK;
}
int ensure_pinned(prach_engine *e, size_t need) {
    if (need <= e->pinned_cap) return PRACH_OK;
    if (e->pinned) HIPCHK(hipHostFree(e->pinned));
    e->pinned = nullptr;
    e->pinned_cap = 0;
    const size_t want = need + (need >> 2) + 4096;
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&e->pinned), want, hipHostMallocDefault));
    e->pinned_cap = want;
    return PRACH_OK;
}

int host_threads(const prach_engine *e) {
    int n = e->opt_host_threads > 0 ? (int)e->opt_host_threads : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(n, 64));
}

// Workgroups of the given cluster launch that can be resident at once on this device: the runtime's occupancy answer for
// the kernel and its dynamic LDS size, times the CU count (MI355X_MICROARCH.md "Residency and cooperative launch": a
// plain launch has the same residency as a cooperative one; the query is what a cooperative launch would check).
int resident_workgroups(const prach_engine *e, int per_cu) {
    if (e->opt_resident > 0) return (int)e->opt_resident;
    return std::max(1, per_cu) * e->num_cus;
}

} // namespace

static int engine_create_impl(int device, prach_engine **out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "[prach] no HIP device: libprach_hip needs an MI355X (gfx950); there is no CPU fallback\n");
        return PRACH_ERR_DEVICE;
    }
    if (device < 0 || device >= ndev) return PRACH_ERR_ARG;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "[prach] device %d is %s; this library is built for gfx950 only\n", device, prop.gcnArchName);
        return PRACH_ERR_DEVICE;
    }
    prach_engine *e = new (std::nothrow) prach_engine();
    if (!e) return PRACH_ERR_DEVICE;
    e->device = device;
    e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    e->mem_budget = (size_t)prop.totalGlobalMem / 4 * 3;
    int rc = [&]() -> int {
        HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&e->ev0));
        HIPCHK(hipEventCreate(&e->ev1));
        return PRACH_OK;
    }();
    if (rc != PRACH_OK) { prach_engine_destroy(e); return rc; } // (nothing half-built is leaked)
    *out = e;
    return PRACH_OK;
}

// LDS-resident records (prach_cluster.hip REC_L16): a Philox cluster whose owned UE slots (the launch's maximum) fit LDS next to
// the per-subframe structures.  Returns the slot count per workgroup, 0 = records stay in global memory.
static int lds_record_slots(const prach_engine *e, const prach_cfg *cfgs, const int *idx, int m, int G, int maxP, int *maxgroups) {
    *maxgroups = 0;
    if (G <= 1 || !e->opt_lds_records || e->opt_dense || cfgs[idx[0]].variant == PRACH_VARIANT_NOMA_C) return 0;
    int lslots = 0;
    for (int k = 0; k < m; k++) {
        const int groups = (cfgs[idx[k]].nUE + 63) / 64;
        lslots = std::max(lslots, (groups + G - 1) / G * 64);
        *maxgroups = std::max(*maxgroups, groups);
    }
    if (cfgs[idx[0]].rng_mode == PRACH_RNG_GLIBC) // the reference's rand() stream: only the lean kernel keeps such a cluster's records in LDS
        return (lslots <= CLUSTER_LQCAP && e->opt_fast && e->opt_pipeline && maxP <= lcluster_max_preambles() && *maxgroups <= lcluster_max_groups_glibc() &&
                lcluster_kernel_lds_bytes(lslots, true, *maxgroups) <= CLUSTER_LDS_LIMIT) ? lslots : 0;
    return (lslots <= CLUSTER_LQCAP && cluster_kernel_lds_bytes(maxP, false, lslots) <= CLUSTER_LDS_LIMIT) ? lslots : 0;
}
// ... on the lean kernel (prach_lcluster.hip): pipelined compacted pass only, nPreamble <= 64
static bool use_fast_kernel(const prach_engine *e, int lslots, int maxP) {
    return lslots > 0 && e->opt_fast && e->opt_pipeline && maxP <= lcluster_max_preambles() && lcluster_kernel_lds_bytes(lslots) <= CLUSTER_LDS_LIMIT;
}

// one workgroup per trial: can prach::batch_kernel (prach_batch.hip) run this trial?  (Philox: both workgroup shapes; the reference's own rand()
// stream: the 1024-thread shape with its per-group call marks in LDS, up to 131 072 UEs)
static bool batch_eligible(const prach_engine *e, const prach_cfg &c) {
    if (c.variant == PRACH_VARIANT_NOMA_C || e->opt_dense || e->opt_wide_records) return false;
    const bool glibc = c.rng_mode == PRACH_RNG_GLIBC;
    return c.nPreamble <= batch_max_preambles() && c.maxRarWindow <= batch_max_rar_window() && batch_calendar_slots(c.backoff, c.accessTime, c.maxRarWindow) <= batch_max_calendar_slots() &&
           (int64_t)prach_max_time(&c) + c.backoff + c.accessTime + 128 < batch_max_subframes() && c.nUE < (1 << 20) - 1 && (c.nUE + 63) / 64 <= batch_max_groups(glibc);
}

// NOMA.c's activeUE table on the device: noma_activation_kernel for every UE of the launch, then the few UEs whose value sits within the
// device math library's error band of a rounding / comparison boundary (~1e-6 of them) are recomputed with the host's libm
// (prach_noma_activation_range) and patched in.  dparams: the launch's TrialDev blocks (device), tabs[k]: trial k's table arrays (device).
struct ActTab { char *pre0, *sec, *gain, *lgain, *nd0; };
constexpr int NOMA_ACT_OVERFLOW_RC = -1099; // (internal) noma_activation_kernel flagged more UEs than its list holds
static int noma_device_activation(prach_engine *e, const TrialDev *dparams, const prach_cfg *cfgs, const int *idx, int m, const std::vector<ActTab> &tabs,
                                  unsigned *dflags, std::vector<std::pair<int, int>> *flagged, int &nflagged) {
    int maxUE = 0;
    for (int k = 0; k < m; k++) maxUE = std::max(maxUE, cfgs[idx[k]].nUE);
    HIPCHK(launch_noma_activation(dparams, m, maxUE, dflags, e->stream));
    unsigned nflag = 0;
    HIPCHK(hipMemcpyAsync(&nflag, dflags, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (nflag > (unsigned)NOMA_ACT_FLAG_CAP) { // (e.g. a cell radius just above the 35 m exclusion zone: the redraw loop's iteration limit flags every tenth UE)
        std::fprintf(stderr, "[prach] noma_activation_kernel flagged %u UEs (more than its list holds): the activation table of this launch is built on the host\n", nflag);
        return NOMA_ACT_OVERFLOW_RC;
    }
    if (!nflag) return PRACH_OK;
    std::vector<unsigned> fl(2 * (size_t)nflag);
    HIPCHK(hipMemcpyAsync(fl.data(), dflags + 2, 8 * (size_t)nflag, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // the recomputed values are staged in buffers that live until the copies have completed ON THE ENGINE'S STREAM (the simulation kernel is launched on that
    // stream, which is non-blocking: a copy on the null stream would not be ordered in front of it)
    struct Patch { int32_t pre0, sec; double gn, lg; uint32_t nd0; };
    std::vector<Patch> pt(nflag);
    for (unsigned q = 0; q < nflag; q++) {
        const int k = (int)fl[2 * q], i = (int)fl[2 * q + 1];
        if (k < 0 || k >= m || i < 0 || i >= cfgs[idx[k]].nUE) return PRACH_ERR_INTERNAL;
        const int arc = prach_noma_activation_range(&cfgs[idx[k]], i, i + 1, &pt[q].pre0, &pt[q].sec, &pt[q].gn, &pt[q].lg, &pt[q].nd0);
        if (arc != PRACH_OK) return arc;
        const ActTab &T = tabs[k];
        HIPCHK(hipMemcpyAsync(T.pre0 + 4 * (size_t)i, &pt[q].pre0, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(T.sec + 4 * (size_t)i, &pt[q].sec, 4, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(T.gain + 8 * (size_t)i, &pt[q].gn, 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(T.lgain + 8 * (size_t)i, &pt[q].lg, 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(T.nd0 + 4 * (size_t)i, &pt[q].nd0, 4, hipMemcpyHostToDevice, e->stream));
        if (flagged) flagged->push_back({k, i});
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    nflagged += (int)nflag;
    return PRACH_OK;
}

// What a call reduces on the device next to its results (prach_run_trials_dist, _timeline, _sojourn, _summary, _trace, _xtab, _pick, _columns, _noma_census, _noma_columns, _noma_summary, _noma_pick).  The call's device buffer is a
// row of parts, [ngroups][words] 64-bit counters each: the arrays the caller gets as they are, one per part, then the scalars the kernel keeps per group,
// which the engine unpacks into the caller's per-group structs.  Every launch of the call gets one job per trial it finished, and the kind's kernel behind
// the simulation kernel.  What differs between the kinds is stated ONCE per kind: a block of functions behind CallCtx and its row of RED_KINDS.  The generic
// code (reduction_begin, run_group, reduction_end, run_trials_impl) walks that row and never asks which kind it has; a new kind is an enumerator, a block and
// a row.  The HOST-SIDE row of a grouped kind (one struct and a few arrays per trial group) is in GROUPED of prach_host.c, stated by csrc/prach_grouped.h: its
// sizes, the shape of its arrays, its spec's judge, the trials it takes, its CSV lines.  There a new grouped kind costs an enumerator, that row, an entry of
// GROUPED_RED below and its three public functions as wrappers; the refusals (prach_internal_grouped_run), merge, CSV dispatch and the CLI's blocks are generic.
enum class Red { dist, timeline, sojourn, summary, trace, xtab, pick, columns, noma_census, noma_columns, noma_summary, noma_pick, noma_trace, noma_timeline, noma_gain };
constexpr int RED_MAX_PARTS = 7;
struct Reduction {
    Red kind;
    const int32_t *group; // nullable: trial k is group k
    int ngroups;
    uint64_t *out[RED_MAX_PARTS - 1]; // the caller's arrays, one per part in front of the scalars
    const void *spec;                 // the caller's prach_*_spec, and its per-group structs (summary: its per-trial rows): the kind's block reads both
    void *groups;                     // through its own casts
    // A BULK PART (bulk_width == 0: none): bulk_rows rows of bulk_width bytes that the kind's kernel writes with plain stores, every byte of them set to
    // bulk_fill once in front of the first launch; what lies between two rows is never touched.  Either the engine owns the device copy (rows without gaps)
    // and copies it out once at the end of the call, to bulk_host, rows bulk_pitch bytes apart — or the part is CALLER-OWNED DEVICE MEMORY, bulk_dev, rows
    // bulk_pitch bytes apart, and the kernel writes straight into it.
    void *bulk_host = nullptr, *bulk_dev = nullptr;
    size_t bulk_width = 0, bulk_rows = 0, bulk_pitch = 0;
    int bulk_fill = 0;
    // A TABLE of the call that the kernel reads (table_bytes == 0: none): uploaded once, behind the counters
    const void *table = nullptr;
    size_t table_bytes = 0;
};
struct CallCtx;
struct JobSrc { const prach_cfg &c; const TrialLayout &L; const DevResult &dr; char *A; int group, wg0; bool batch; }; // a finished trial of a launch, as a job is filled from it (A: the arena)
struct RedKind {
    int (*parts)(const Reduction &, size_t words[RED_MAX_PARTS]); // words per group of every part, the scalars last; returns their number
    size_t job_bytes; int tile;               // tile: UEs or subframes per workgroup
    int (*fill_job)(void *job, const JobSrc &); // returns the trial's UEs or subframes: it takes ceil(that / tile) workgroups from wg0 on
    bool device_logs, trace_rows, fast_off;   // every trial needs a device log region / trace rows; the call takes the paths that "fast" = 0 takes
    hipError_t (*launch)(const prach_engine *e, const Reduction &, int njobs, int wgs, unsigned long long *const *d); // (jobs: e->red_jobs_d, on the host e->red_jobs_h)
    void (*empty)(const Reduction &, size_t g, const prach_cfg *cfgs); // the caller's struct of group g before anything ran
    int (*unpack)(const Reduction &, CallCtx &, size_t g, const unsigned long long *q); // ... and from the group's scalar words at the end of the call
    double prach_timing::*ms;                 // where the kernel time of the call goes
    // a kind whose kernel needs something prepared per launch, behind the jobs' upload and in front of the kernel (nullptr: nothing): the jobs of the accepted
    // trials are on the device (and at e->red_jobs_h); `levels`: every NOMA.c trial of the call's launches gets a level column and the launch a list of EDGE UEs
    int (*prepass)(prach_engine *e, CallCtx &, const std::vector<JobSrc> &acc, int njobs, int wgs) = nullptr;
    bool levels = false;
};
const RedKind &kind_of(const Reduction &r);

// What one prach_run_trials call carries from launch to launch
struct CallCtx {
    const prach_cfg *cfgs;
    prach_result *results;
    prach_ue_log *const *ue_logs;
    double kernel_ms = 0, upload_ms = 0;
    int noma_flagged = 0, noma_ambiguous = 0; // UEs recomputed on the host, trials rerun with the host-built table
    int gain_host_ues = 0;                    // prach_run_trials_noma_gain: UEs whose level the host resolved
    // the call's reduction (red == nullptr: plain prach_run_trials, nothing below is touched)
    const Reduction *red = nullptr;
    double red_ms = 0;
    unsigned long long *d_part[RED_MAX_PARTS] = {}; // the call's device buffer, part by part (red_parts)
    std::vector<uint64_t> trials, ues;        // per group, counted on the host as launches are accepted
    int group_of(int k) const { return red->group ? red->group[k] : k; }
    bool reads_device_logs() const { return red && kind_of(*red).device_logs; }
    bool traces() const { return red && kind_of(*red).trace_rows; }
    bool levels() const { return red && kind_of(*red).levels; }
};
// ---- the kinds of reduction, one block each --------------------------------------------------------------------------------------------------------------
template <class T> const T &spec_of(const Reduction &r) { return *static_cast<const T *>(r.spec); }
template <class T> T &group_of(const Reduction &r, size_t g) { return static_cast<T *>(r.groups)[g]; }
// the caller's struct of a group before anything ran: zeros, and -1 where a maximum over nothing stands
template <class T, int64_t T::*...MAX> void empty_group(const Reduction &r, size_t g, const prach_cfg *) { T &t = group_of<T>(r, g); t = T{}; ((t.*MAX = -1), ...); }
// prach_result.steps of a finished trial: what the kernel counted, except where every UE of a NOMA.c trial succeeded — NOMA.c:707-710 breaks behind the last
// success, prach::noma_kernel sees that only at a slot head (or not at all before `stop`), and dbg[0] holds the latest success subframe + 1
unsigned long long steps_of(const prach_cfg &c, const DevResult &dr) {
    return c.variant == PRACH_VARIANT_NOMA_C && dr.nSuccess == c.nUE && dr.dbg[0] > 0 ? dr.dbg[0] : dr.steps;
}
int subframes_run(const JobSrc &s) { return (int)std::min<unsigned long long>(steps_of(s.c, s.dr), (unsigned long long)prach_max_time(&s.c)); } // E of include/prach.h: from prach_result.steps
// timeline, sojourn, summary, xtab and pick read a trial's log records and the launch's own copy of its arrival schedule; STEPS (xtab, pick): E of include/prach.h in the last word
template <bool STEPS> int fill_timeline_job(void *job, const JobSrc &s) {
    const int nslots = (prach_max_time(&s.c) + s.c.accessTime - 1) / s.c.accessTime; // (what prach_arrival_schedule fills; the table has one entry more)
    *static_cast<TimelineJob *>(job) = TimelineJob{reinterpret_cast<const int4 *>(s.A + s.L.logs), reinterpret_cast<const int *>(s.A + s.L.sched), s.c.nUE, s.group, s.wg0, s.c.accessTime, nslots,
                                                   STEPS ? subframes_run(s) : 0};
    return s.c.nUE;
}
const TimelineJob *timeline_jobs(const prach_engine *e) { return reinterpret_cast<const TimelineJob *>(e->red_jobs_d); }

// dist: delay_hist, ptc_hist | scalars; reads the timers and preamble counts the simulation kernel left in the arena
int dist_parts(const Reduction &r, size_t w[]) { w[0] = (size_t)spec_of<prach_dist_spec>(r).delay_bins; w[1] = PRACH_DIST_PTC_BINS; w[2] = DIST_SCALARS; return 3; }
int dist_fill_job(void *job, const JobSrc &s) {
    *static_cast<DistJob *>(job) = DistJob{reinterpret_cast<const int *>(s.A + s.L.timers), reinterpret_cast<const int *>(s.A + (s.batch ? s.L.rec32 : s.L.ptc)), s.c.nUE, s.group, s.wg0, s.batch ? 1 : 0};
    return s.c.nUE;
}
hipError_t dist_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_dist_spec &sp = spec_of<prach_dist_spec>(r);
    return launch_dist_kernel(reinterpret_cast<const DistJob *>(e->red_jobs_d), njobs, wgs, sp.delay_bins, sp.delay_bin_ms, (int)e->opt_dist_scheme, d[0], d[1], d[2], e->stream);
}
int dist_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_dist &d = group_of<prach_dist>(r, g);
    d.trials = cx.trials[g]; d.ues = cx.ues[g]; d.success = q[0]; d.delay_overflow = q[1]; d.delay_sum = q[2]; d.ptc_sum = q[3]; d.delay_max = (int64_t)q[4] - 1;
    return PRACH_OK;
}

// timeline: the five series arrivals, success, sojourn_sum, timer_sum, done | scalars
int timeline_parts(const Reduction &r, size_t w[]) { for (int q = 0; q < 5; q++) w[q] = (size_t)spec_of<prach_timeline_spec>(r).bins; w[5] = TL_SCALARS; return 6; }
hipError_t timeline_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_timeline_spec &sp = spec_of<prach_timeline_spec>(r);
    return launch_timeline_kernel(timeline_jobs(e), njobs, wgs, sp.bins, sp.bin_ms, (int)e->opt_timeline_scheme, TimelineOut{d[0], d[1], d[2], d[3], d[4], d[5]}, e->stream);
}
int timeline_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_timeline &t = group_of<prach_timeline>(r, g);
    t.trials = cx.trials[g]; t.ues = cx.ues[g]; t.arrived = q[0]; t.success = q[1]; t.restarted = q[2]; t.arrival_overflow = q[3]; t.done_overflow = q[4];
    t.sojourn_sum = q[5]; t.timer_sum = q[6]; t.done_max = (int64_t)q[7] - 1;
    return PRACH_OK;
}

// sojourn: hist, row_arrived, row_delay_overflow | scalars
int sojourn_parts(const Reduction &r, size_t w[]) {
    const prach_sojourn_spec &sp = spec_of<prach_sojourn_spec>(r);
    w[0] = (size_t)sp.arrival_bins * (size_t)sp.delay_bins; w[1] = w[2] = (size_t)sp.arrival_bins; w[3] = SJ_SCALARS;
    return 4;
}
hipError_t sojourn_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_sojourn_spec &sp = spec_of<prach_sojourn_spec>(r);
    return launch_sojourn_kernel(timeline_jobs(e), njobs, wgs, sp.arrival_bins, sp.arrival_bin_ms, sp.delay_bins, sp.delay_bin_ms, (int)e->opt_sojourn_scheme, SojournOut{d[0], d[1], d[2], d[3]}, e->stream);
}
int sojourn_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_sojourn &j = group_of<prach_sojourn>(r, g);
    j.trials = cx.trials[g]; j.ues = cx.ues[g]; j.arrived = q[0]; j.success = q[1]; j.restarted = q[2]; j.arrival_overflow = q[3]; j.delay_overflow = q[4];
    j.sojourn_sum = q[5]; j.sojourn_max = (int64_t)q[6] - 1;
    return PRACH_OK;
}

// summary: every trial is its own group, and the only part is the kernel's row of SM_WORDS words per trial; ONE workgroup per job, whatever the tile
int summary_parts(const Reduction &, size_t w[]) { w[0] = SM_WORDS; return 1; }
hipError_t summary_launch(const prach_engine *e, const Reduction &r, int njobs, int, unsigned long long *const *d) {
    const prach_summary_spec &sp = spec_of<prach_summary_spec>(r);
    SummaryLevels lv{};
    lv.nq = sp.nq;
    for (int l = 0; l < lv.nq; l++) lv.permille[l] = sp.permille[l];
    int max_slots = 0; // the longest schedule of the jobs
    for (int j = 0; j < njobs; j++) max_slots = std::max(max_slots, reinterpret_cast<const TimelineJob *>(e->red_jobs_h)[j].nslots);
    return launch_summary_kernel(timeline_jobs(e), njobs, lv, (int)e->opt_summary_threads, std::min(max_slots, summary_sched_cap()), d[0], e->stream);
}
void summary_empty(const Reduction &r, size_t k, const prach_cfg *cfgs) {
    prach_trial_summary &row = group_of<prach_trial_summary>(r, k);
    std::memset(&row, 0, sizeof(row));
    row.status = PRACH_ERR_INTERNAL;
    row.nUE = cfgs[k].nUE;
    row.sojourn_max = row.timer_max = row.ptc_max = -1;
    std::memset(row.q, 0xff, sizeof(row.q)); // -1
}
int summary_unpack(const Reduction &r, CallCtx &cx, size_t k, const unsigned long long *words) { // status and nUE from the host, the rest from the one launch that accepted the trial
    prach_trial_summary &row = group_of<prach_trial_summary>(r, k);
    row.status = cx.results[k].status; // (everything else is still the empty row)
    if (row.status != PRACH_OK) return PRACH_OK;
    if (cx.trials[k] != 1) return row.status = PRACH_ERR_INTERNAL; // (no launch reduced this trial, or two did)
    const long long *const q = reinterpret_cast<const long long *>(words);
    row.arrived = (int32_t)q[0]; row.success = (int32_t)q[1]; row.restarted = (int32_t)q[2];
    row.range_errors = (int32_t)std::min<long long>(q[3] + q[4] + q[5], INT32_MAX);
    row.sojourn_sum = q[6]; row.timer_sum = q[7]; row.ptc_sum = q[8];
    row.sojourn_max = (int32_t)q[9]; row.timer_max = (int32_t)q[10]; row.ptc_max = (int32_t)q[11];
    for (int x = 0; x < 3; x++)
        for (int l = 0; l < spec_of<prach_summary_spec>(r).nq; l++) row.q[x][l] = q[3 + x] ? -1 : (int32_t)q[12 + x * PRACH_SUMMARY_MAX_Q + l];
    return row.range_errors ? PRACH_ERR_INTERNAL : PRACH_OK; // (a value the kernel cannot rank: no trial produces one)
}

// trace: the four series calls, singles, txop, collisions | scalars; reads the rows the simulation kernels write per subframe, which prach::lcluster_kernel does
// not (its source and its speed stay what they are): the call takes the paths that "fast" = 0 takes
int trace_parts(const Reduction &r, size_t w[]) { for (int q = 0; q < 4; q++) w[q] = (size_t)spec_of<prach_trace_spec>(r).bins; w[4] = TR_SCALARS; return 5; }
int trace_fill_job(void *job, const JobSrc &s) { // the rows of the subframes [0, steps): what this launch's kernel wrote for the trial, and the zeros behind time_exit are never read
    const int steps = subframes_run(s);
    *static_cast<TraceJob *>(job) = TraceJob{reinterpret_cast<const int4 *>(s.A + s.L.trace), steps, s.group, s.wg0, 0};
    return steps;
}
hipError_t trace_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_trace_spec &sp = spec_of<prach_trace_spec>(r);
    return launch_trace_kernel(reinterpret_cast<const TraceJob *>(e->red_jobs_d), njobs, wgs, sp.bins, sp.bin_ms, (int)e->opt_trace_scheme, TraceOut{d[0], d[1], d[2], d[3], d[4]}, e->stream);
}
int trace_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_trace &t = group_of<prach_trace>(r, g);
    t.trials = cx.trials[g]; t.subframes = q[0]; t.calls = q[1]; t.singles = q[2]; t.txop = q[3]; t.collisions = q[4]; t.overflow_calls = q[5]; t.calls_max = (int64_t)q[6] - 1;
    return PRACH_OK;
}

// xtab: cells | scalars; the timeline's jobs with E = min(steps, maxTime) in their last word
int xtab_parts(const Reduction &r, size_t w[]) {
    const prach_xtab_spec &x = spec_of<prach_xtab_spec>(r);
    w[0] = ((size_t)x.row_bins + 1) * ((size_t)x.col_bins + 1); w[1] = XT_SCALARS;
    return 2;
}
hipError_t xtab_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_xtab_spec &x = spec_of<prach_xtab_spec>(r);
    return launch_xtab_kernel(timeline_jobs(e), njobs, wgs, XtabAxes{x.who, x.row_field, x.row_width, x.row_bins, x.col_field, x.col_width, x.col_bins}, (int)e->opt_xtab_scheme, XtabOut{d[0], d[1]}, e->stream);
}
int xtab_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_xtab &x = group_of<prach_xtab>(r, g);
    x.trials = cx.trials[g]; x.ues = cx.ues[g]; x.idle = q[0]; x.served = q[1]; x.unserved = q[2]; x.selected = q[3]; x.binned = q[4];
    x.undefined = q[3] - q[4]; x.row_sum = q[5]; x.col_sum = q[6]; x.row_max = (int64_t)q[7] - 1; x.col_max = (int64_t)q[8] - 1;
    return PRACH_OK;
}

// pick: every trial is its own group, as in the summary; the rows, k x PK_ROW_WORDS words per trial, go to the caller as they are and are then sorted in
// place, trial by trial, into the defined order (the kernel leaves them in UE-index order: prach_pick.hip) | scalars; ONE workgroup per job
int pick_parts(const Reduction &r, size_t w[]) { w[0] = (size_t)spec_of<prach_pick_spec>(r).k * PK_ROW_WORDS; w[1] = PK_SCALARS; return 2; }
hipError_t pick_launch(const prach_engine *e, const Reduction &r, int njobs, int, unsigned long long *const *d) {
    int max_slots = 0; // the longest schedule of the jobs
    for (int j = 0; j < njobs; j++) max_slots = std::max(max_slots, reinterpret_cast<const TimelineJob *>(e->red_jobs_h)[j].nslots);
    return launch_pick_kernel(timeline_jobs(e), njobs, spec_of<prach_pick_spec>(r), (int)e->opt_pick_threads, std::min(max_slots, pick_sched_cap()), d[0], d[1], e->stream);
}
void pick_empty(const Reduction &r, size_t t, const prach_cfg *cfgs) {
    prach_pick &h = group_of<prach_pick>(r, t);
    h = prach_pick{};
    h.status = PRACH_ERR_INTERNAL;
    h.nUE = cfgs[t].nUE;
    h.threshold = -1;
}
int pick_unpack(const Reduction &r, CallCtx &cx, size_t t, const unsigned long long *words) { // status and nUE from the host, the rest from the one launch that accepted the trial
    const prach_pick_spec &sp = spec_of<prach_pick_spec>(r);
    prach_pick &h = group_of<prach_pick>(r, t);
    prach_pick_row *const rows = reinterpret_cast<prach_pick_row *>(r.out[0]) + t * (size_t)sp.k;
    h.status = cx.results[t].status; // (everything else is still the empty header, and no launch wrote a row of a trial it did not accept)
    if (h.status != PRACH_OK) return PRACH_OK;
    const long long *const q = reinterpret_cast<const long long *>(words);
    if (cx.trials[t] != 1 || q[2] < 0 || q[2] > sp.k) { // (no launch picked from this trial, or two did)
        std::memset(rows, 0, sizeof(prach_pick_row) * (size_t)sp.k);
        return h.status = PRACH_ERR_INTERNAL;
    }
    h.selected = (int32_t)q[0]; h.matched = (int32_t)q[1]; h.undefined = (int32_t)q[3]; h.range_errors = (int32_t)q[4];
    if (h.range_errors) { // (a key the kernel cannot rank: no trial produces one) the rows are void
        std::memset(rows, 0, sizeof(prach_pick_row) * (size_t)sp.k);
        return PRACH_ERR_INTERNAL;
    }
    h.stored = (int32_t)q[2]; h.threshold = (int32_t)q[5]; h.ties_left_out = (int32_t)q[6];
    // stable: equal keys stay in ascending UE index
    if (sp.order == PRACH_PICK_LARGEST) std::stable_sort(rows, rows + h.stored, [](const prach_pick_row &a, const prach_pick_row &b) { return a.key > b.key; });
    if (sp.order == PRACH_PICK_SMALLEST) std::stable_sort(rows, rows + h.stored, [](const prach_pick_row &a, const prach_pick_row &b) { return a.key < b.key; });
    return PRACH_OK;
}

// columns: every trial is its own group, as in the summary; the columns are the call's bulk part, ncols rows of (sum of nUE) words, and the table is the first
// row of every trial; the only counters are the scalars: the three class counts of a trial
int columns_parts(const Reduction &, size_t w[]) { w[0] = CL_SCALARS; return 1; }
hipError_t columns_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    return launch_columns_kernel(timeline_jobs(e), njobs, wgs, spec_of<prach_columns_spec>(r),
                                 ColumnsOut{reinterpret_cast<int *>(e->red_bulk), e->red_bulk_pitch / 4, reinterpret_cast<const unsigned long long *>(e->red_table), d[0]}, e->stream);
}
void columns_empty(const Reduction &r, size_t k, const prach_cfg *cfgs) {
    prach_columns &h = group_of<prach_columns>(r, k);
    h = prach_columns{};
    h.status = PRACH_ERR_INTERNAL;
    h.nUE = cfgs[k].nUE;
    h.offset = static_cast<const uint64_t *>(r.table)[k];
}
int columns_unpack(const Reduction &r, CallCtx &cx, size_t k, const unsigned long long *q) { // status and nUE from the host, the counts from the one launch that accepted the trial
    prach_columns &h = group_of<prach_columns>(r, k);
    h.status = cx.results[k].status; // (everything else is still the empty header, and no launch wrote a word of a trial it did not accept)
    if (h.status != PRACH_OK) return PRACH_OK;
    if (cx.trials[k] != 1 || q[0] + q[1] + q[2] != (unsigned long long)h.nUE) return h.status = PRACH_ERR_INTERNAL; // (no launch wrote this trial, or two did)
    h.idle = (int32_t)q[0]; h.served = (int32_t)q[1]; h.unserved = (int32_t)q[2];
    return PRACH_OK;
}

// noma_census: xtab's parts and jobs with the NOMA menu (prach_noma_census.hip): cells | scalars, one class more
int noma_census_parts(const Reduction &r, size_t w[]) {
    const prach_xtab_spec &x = spec_of<prach_xtab_spec>(r);
    w[0] = ((size_t)x.row_bins + 1) * ((size_t)x.col_bins + 1); w[1] = NC_SCALARS;
    return 2;
}
hipError_t noma_census_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_xtab_spec &x = spec_of<prach_xtab_spec>(r);
    return launch_noma_census_kernel(timeline_jobs(e), njobs, wgs, XtabAxes{x.who, x.row_field, x.row_width, x.row_bins, x.col_field, x.col_width, x.col_bins}, (int)e->opt_xtab_scheme, XtabOut{d[0], d[1]}, e->stream);
}
int noma_census_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_noma_census &x = group_of<prach_noma_census>(r, g);
    x.trials = cx.trials[g]; x.ues = cx.ues[g]; x.idle = q[0]; x.served = q[1]; x.dropped = q[2]; x.pending = q[3]; x.selected = q[4]; x.binned = q[5];
    x.undefined = q[4] - q[5]; x.row_sum = q[6]; x.col_sum = q[7]; x.row_max = (int64_t)q[8] - 1; x.col_max = (int64_t)q[9] - 1;
    return PRACH_OK;
}

// noma_columns: the columns' bulk part and table with the NOMA menu; the scalars are the four class counts of a trial
int noma_columns_parts(const Reduction &, size_t w[]) { w[0] = NCL_SCALARS; return 1; }
hipError_t noma_columns_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    return launch_noma_columns_kernel(timeline_jobs(e), njobs, wgs, spec_of<prach_columns_spec>(r),
                                      ColumnsOut{reinterpret_cast<int *>(e->red_bulk), e->red_bulk_pitch / 4, reinterpret_cast<const unsigned long long *>(e->red_table), d[0]}, e->stream);
}
void noma_columns_empty(const Reduction &r, size_t k, const prach_cfg *cfgs) {
    prach_noma_columns &h = group_of<prach_noma_columns>(r, k);
    h = prach_noma_columns{};
    h.status = PRACH_ERR_INTERNAL;
    h.nUE = cfgs[k].nUE;
    h.offset = static_cast<const uint64_t *>(r.table)[k];
}
int noma_columns_unpack(const Reduction &r, CallCtx &cx, size_t k, const unsigned long long *q) { // status and nUE from the host, the counts from the one launch that accepted the trial
    prach_noma_columns &h = group_of<prach_noma_columns>(r, k);
    h.status = cx.results[k].status; // (everything else is still the empty header, and no launch wrote a word of a trial it did not accept)
    if (h.status != PRACH_OK) return PRACH_OK;
    if (cx.trials[k] != 1 || q[0] + q[1] + q[2] + q[3] != (unsigned long long)h.nUE) return h.status = PRACH_ERR_INTERNAL; // (no launch wrote this trial, or two did)
    h.idle = (int32_t)q[0]; h.served = (int32_t)q[1]; h.dropped = (int32_t)q[2]; h.pending = (int32_t)q[3];
    return PRACH_OK;
}

// noma_summary: every trial is its own group, and the only part is the kernel's row of NSM_WORDS words per trial (prach_noma_select.hip); the unpack follows
// summary's.  ONE workgroup per job; the workgroup size is the summary's option ("summary_threads"): taken over from summary_kernel, NOT measured for this kernel
int noma_summary_parts(const Reduction &, size_t w[]) { w[0] = NSM_WORDS; return 1; }
hipError_t noma_summary_launch(const prach_engine *e, const Reduction &r, int njobs, int, unsigned long long *const *d) {
    int max_slots = 0; // the longest schedule of the jobs
    for (int j = 0; j < njobs; j++) max_slots = std::max(max_slots, reinterpret_cast<const TimelineJob *>(e->red_jobs_h)[j].nslots);
    return launch_noma_summary_kernel(timeline_jobs(e), njobs, spec_of<prach_noma_summary_spec>(r), (int)e->opt_summary_threads, std::min(max_slots, noma_select_sched_cap()), d[0], e->stream);
}
void noma_summary_empty(const Reduction &r, size_t k, const prach_cfg *cfgs) {
    prach_noma_trial_summary &row = group_of<prach_noma_trial_summary>(r, k);
    std::memset(&row, 0, sizeof(row));
    row.status = PRACH_ERR_INTERNAL;
    row.nUE = cfgs[k].nUE;
    std::memset(row.max, 0xff, sizeof(row.max)); // -1
    std::memset(row.q, 0xff, sizeof(row.q));
}
int noma_summary_unpack(const Reduction &r, CallCtx &cx, size_t k, const unsigned long long *words) { // status and nUE from the host, the rest from the one launch that accepted the trial
    const prach_noma_summary_spec &sp = spec_of<prach_noma_summary_spec>(r);
    prach_noma_trial_summary &row = group_of<prach_noma_trial_summary>(r, k);
    row.status = cx.results[k].status; // (everything else is still the empty row)
    if (row.status != PRACH_OK) return PRACH_OK;
    const long long *const q = reinterpret_cast<const long long *>(words);
    if (cx.trials[k] != 1 || q[0] + q[1] + q[2] + q[3] != (long long)row.nUE) return row.status = PRACH_ERR_INTERNAL; // (no launch reduced this trial, or two did)
    row.idle = (int32_t)q[0]; row.served = (int32_t)q[1]; row.dropped = (int32_t)q[2]; row.pending = (int32_t)q[3]; row.selected = (int32_t)q[4]; row.restarted = (int32_t)q[5];
    long long rerr = 0;
    for (int x = 0; x < sp.nfields; x++) {
        rerr += q[6 + x];
        row.n[x] = (int32_t)q[10 + x]; row.sum[x] = q[14 + x]; row.max[x] = (int32_t)q[18 + x];
        for (int l = 0; l < sp.nq; l++) row.q[x][l] = q[6 + x] ? -1 : (int32_t)q[22 + x * PRACH_SUMMARY_MAX_Q + l];
    }
    row.range_errors = (int32_t)std::min<long long>(rerr, INT32_MAX);
    return row.range_errors ? PRACH_ERR_INTERNAL : PRACH_OK; // (a value the kernel cannot rank: no trial produces one)
}

// noma_pick: pick's parts, empty header, unpack and host sort with the NOMA menu's kernel (prach_noma_select.hip).  The workgroup size is pick's option
// ("pick_threads", 1024 by default): taken over from pick_kernel, NOT measured for this kernel
hipError_t noma_pick_launch(const prach_engine *e, const Reduction &r, int njobs, int, unsigned long long *const *d) {
    int max_slots = 0; // the longest schedule of the jobs
    for (int j = 0; j < njobs; j++) max_slots = std::max(max_slots, reinterpret_cast<const TimelineJob *>(e->red_jobs_h)[j].nslots);
    return launch_noma_pick_kernel(timeline_jobs(e), njobs, spec_of<prach_pick_spec>(r), (int)e->opt_pick_threads, std::min(max_slots, noma_select_sched_cap()), d[0], d[1], e->stream);
}

// noma_trace: the six series tx, used, singles, granted, pairs, pair_one, [6 sectors][bins] per group | scalars; reads the rows prach::noma_kernel writes per
// (access slot, sector) — of the slots whose subframe lies in [0, steps): what this launch's kernel wrote for the trial, and the zeros behind an early exit
int noma_trace_parts(const Reduction &r, size_t w[]) { for (int q = 0; q < 6; q++) w[q] = 6 * (size_t)spec_of<prach_noma_trace_spec>(r).bins; w[6] = NT_SCALARS; return 7; }
int noma_trace_fill_job(void *job, const JobSrc &s) {
    const int nrows = 6 * ((subframes_run(s) + s.c.accessTime - 1) / s.c.accessTime);
    *static_cast<NomaTraceJob *>(job) = NomaTraceJob{reinterpret_cast<const int4 *>(s.A + s.L.trace), nrows, s.group, s.wg0, s.c.accessTime};
    return nrows;
}
hipError_t noma_trace_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_noma_trace_spec &sp = spec_of<prach_noma_trace_spec>(r);
    return launch_noma_trace_kernel(reinterpret_cast<const NomaTraceJob *>(e->red_jobs_d), njobs, wgs, sp.bins, sp.bin_ms, (int)e->opt_trace_scheme,
                                    NomaTraceOut{{d[0], d[1], d[2], d[3], d[4], d[5]}, d[6]}, e->stream);
}
int noma_trace_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_noma_trace &t = group_of<prach_noma_trace>(r, g);
    t.trials = cx.trials[g]; t.slots = q[0]; t.tx = q[1]; t.used = q[2]; t.singles = q[3]; t.granted = q[4]; t.pairs = q[5]; t.pair_one = q[6]; t.overflow_tx = q[7];
    t.tx_max = (int64_t)q[8] - 1;
    return PRACH_OK;
}

// noma_timeline: the six series arrivals, served, dropped, sojourn_sum, timer_sum, done, [6 sectors][bins] per group | scalars; reads the log records
// prach::noma_kernel leaves on the device, the launch's schedule and E (prach_noma_timeline.hip)
int noma_timeline_parts(const Reduction &r, size_t w[]) { for (int q = 0; q < 6; q++) w[q] = 6 * (size_t)spec_of<prach_noma_timeline_spec>(r).bins; w[6] = NTL_SCALARS; return 7; }
hipError_t noma_timeline_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_noma_timeline_spec &sp = spec_of<prach_noma_timeline_spec>(r);
    return launch_noma_timeline_kernel(timeline_jobs(e), njobs, wgs, sp.bins, sp.bin_ms, (int)e->opt_timeline_scheme, (int)e->opt_noma_timeline_window,
                                       NomaTimelineOut{{d[0], d[1], d[2], d[3], d[4], d[5]}, d[6]}, e->stream);
}
int noma_timeline_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_noma_timeline &t = group_of<prach_noma_timeline>(r, g);
    t.trials = cx.trials[g]; t.ues = cx.ues[g]; t.idle = q[0]; t.served = q[1]; t.dropped = q[2]; t.pending = q[3]; t.undefined = q[4]; t.restarted = q[5];
    t.arrival_overflow = q[6]; t.done_overflow = q[7]; t.sojourn_sum = q[8]; t.timer_sum = q[9]; t.done_max = (int64_t)q[10] - 1;
    return PRACH_OK;
}

template <class F> static void parallel_for(int nth, size_t n, const F &f); // (below)

// noma_gain: the six series arrived, served, dropped, sojourn_sum, lost_sum, ptc_sum, [6 sectors][bins] per group | scalars; reads the log records, the launch's
// schedule and E like the NOMA timeline, and the level column its pre-pass fills from the launch's activation table (prach_noma_gain.hip)
int noma_gain_parts(const Reduction &r, size_t w[]) { for (int q = 0; q < 6; q++) w[q] = 6 * (size_t)spec_of<prach_noma_gain_spec>(r).bins; w[6] = NG_SCALARS; return 7; }
int noma_gain_fill_job(void *job, const JobSrc &s) {
    NomaGainJob *const j = static_cast<NomaGainJob *>(job);
    const int n = fill_timeline_job<true>(static_cast<TimelineJob *>(j), s);
    j->lgain = reinterpret_cast<const double *>(s.A + s.L.n_lgain);
    j->level = reinterpret_cast<int *>(s.A + s.L.n_level);
    return n;
}
// The level pre-pass of a launch's accepted trials, then the host's part: the listed EDGE UEs are recomputed with the host's libm (prach_noma_activation_range,
// prach_noma_gain_level) and their 4-byte levels patched into the column — as noma_device_activation patches the activation table; when the list overflowed,
// every level of the launch is built on the host, never silently.  On the engine's stream, completed on return: the reducer starts behind it.
int noma_gain_prepass(prach_engine *e, CallCtx &cx, const std::vector<JobSrc> &acc, int njobs, int wgs) {
    if (njobs != (int)acc.size() || !acc[0].L.gain_edges) return PRACH_ERR_INTERNAL;
    for (const JobSrc &s : acc) if (!s.L.n_level || !s.L.n_lgain) return PRACH_ERR_INTERNAL; // (a launch that laid out no level column: not a NOMA.c Philox launch)
    unsigned *const dedges = reinterpret_cast<unsigned *>(acc[0].A + acc[0].L.gain_edges);
    HIPCHK(launch_noma_gain_levels(reinterpret_cast<const NomaGainJob *>(e->red_jobs_d), njobs, wgs, dedges, NG_EDGE_CAP, e->stream));
    unsigned nedge = 0;
    HIPCHK(hipMemcpyAsync(&nedge, dedges, 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (!nedge) return PRACH_OK;
    struct Act { int32_t pre0, sec; double gn, lg; uint32_t nd0; };
    if (nedge > (unsigned)NG_EDGE_CAP) {
        std::fprintf(stderr, "[prach] the gain-level pre-pass listed %u UEs (more than its list holds): the levels of this launch are built on the host\n", nedge);
        for (const JobSrc &s : acc) {
            std::vector<int32_t> lv((size_t)s.c.nUE);
            const int step = 4096;
            std::vector<int> rcs((size_t)(s.c.nUE + step - 1) / step, PRACH_OK);
            parallel_for(host_threads(e), rcs.size(), [&](size_t q) {
                const int lo = (int)q * step, hi = std::min(s.c.nUE, lo + step);
                std::vector<Act> a((size_t)(hi - lo));
                for (int i = lo; i < hi && rcs[q] == PRACH_OK; i++) {
                    Act &x = a[(size_t)(i - lo)];
                    rcs[q] = prach_noma_activation_range(&s.c, i, i + 1, &x.pre0, &x.sec, &x.gn, &x.lg, &x.nd0);
                    lv[(size_t)i] = prach_noma_gain_level(x.lg);
                }
            });
            for (int rc : rcs) if (rc != PRACH_OK) return rc;
            HIPCHK(hipMemcpyAsync(s.A + s.L.n_level, lv.data(), 4 * lv.size(), hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream)); // (lv is pageable host memory that goes away)
            cx.gain_host_ues += s.c.nUE;
        }
        return PRACH_OK;
    }
    std::vector<unsigned> ed(2 * (size_t)nedge);
    HIPCHK(hipMemcpyAsync(ed.data(), dedges + 2, 8 * (size_t)nedge, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<int32_t> lv(nedge); // (staged until the copies have completed on the engine's stream)
    for (unsigned q = 0; q < nedge; q++) {
        const int j = (int)ed[2 * q], i = (int)ed[2 * q + 1];
        if (j < 0 || j >= njobs || i < 0 || i >= acc[(size_t)j].c.nUE) return PRACH_ERR_INTERNAL;
        const JobSrc &s = acc[(size_t)j];
        Act x;
        const int arc = prach_noma_activation_range(&s.c, i, i + 1, &x.pre0, &x.sec, &x.gn, &x.lg, &x.nd0);
        if (arc != PRACH_OK) return arc;
        lv[q] = prach_noma_gain_level(x.lg);
        HIPCHK(hipMemcpyAsync(s.A + s.L.n_level + 4 * (size_t)i, &lv[q], 4, hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    cx.gain_host_ues += (int)nedge;
    return PRACH_OK;
}
hipError_t noma_gain_launch(const prach_engine *e, const Reduction &r, int njobs, int wgs, unsigned long long *const *d) {
    const prach_noma_gain_spec &sp = spec_of<prach_noma_gain_spec>(r);
    return launch_noma_gain_kernel(reinterpret_cast<const NomaGainJob *>(e->red_jobs_d), njobs, wgs, sp.bins, sp.width, sp.lo, (int)e->opt_timeline_scheme,
                                   NomaGainOut{{d[0], d[1], d[2], d[3], d[4], d[5]}, d[6]}, e->stream);
}
int noma_gain_unpack(const Reduction &r, CallCtx &cx, size_t g, const unsigned long long *q) {
    prach_noma_gain &t = group_of<prach_noma_gain>(r, g);
    t.trials = cx.trials[g]; t.ues = cx.ues[g]; t.idle = q[0]; t.served = q[1]; t.dropped = q[2]; t.pending = q[3]; t.undefined = q[4]; t.below = q[5]; t.above = q[6];
    t.restarted = q[7]; t.sojourn_sum = q[8]; t.lost_sum = q[9]; t.ptc_sum = q[10]; t.defined = q[11];
    t.level_max = q[11] ? (int64_t)q[12] - (1ll << 31) : -1;
    t.neg_level_max = q[11] ? (int64_t)q[13] - (1ll << 31) : -1;
    return PRACH_OK;
}

// in the order of enum class Red:           parts, job bytes, tile, job, device logs, trace rows, "fast" off, launch, empty, unpack, prach_timing field
const RedKind RED_KINDS[] = {
    {dist_parts, sizeof(DistJob), DIST_TILE, dist_fill_job, false, false, false, dist_launch, empty_group<prach_dist, &prach_dist::delay_max>, dist_unpack, &prach_timing::dist_ms},
    {timeline_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<false>, true, false, false, timeline_launch, empty_group<prach_timeline, &prach_timeline::done_max>, timeline_unpack, &prach_timing::timeline_ms},
    {sojourn_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<false>, true, false, false, sojourn_launch, empty_group<prach_sojourn, &prach_sojourn::sojourn_max>, sojourn_unpack, &prach_timing::sojourn_ms},
    {summary_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<false>, true, false, false, summary_launch, summary_empty, summary_unpack, &prach_timing::summary_ms},
    {trace_parts, sizeof(TraceJob), TR_TILE, trace_fill_job, false, true, true, trace_launch, empty_group<prach_trace, &prach_trace::calls_max>, trace_unpack, &prach_timing::trace_ms},
    {xtab_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, xtab_launch, empty_group<prach_xtab, &prach_xtab::row_max, &prach_xtab::col_max>, xtab_unpack, &prach_timing::xtab_ms},
    {pick_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, pick_launch, pick_empty, pick_unpack, &prach_timing::pick_ms},
    {columns_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, columns_launch, columns_empty, columns_unpack, &prach_timing::columns_ms},
    {noma_census_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, noma_census_launch, empty_group<prach_noma_census, &prach_noma_census::row_max, &prach_noma_census::col_max>, noma_census_unpack, &prach_timing::noma_census_ms},
    {noma_columns_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, noma_columns_launch, noma_columns_empty, noma_columns_unpack, &prach_timing::noma_columns_ms},
    {noma_summary_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, noma_summary_launch, noma_summary_empty, noma_summary_unpack, &prach_timing::noma_summary_ms},
    {pick_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, noma_pick_launch, pick_empty, pick_unpack, &prach_timing::noma_pick_ms},
    {noma_trace_parts, sizeof(NomaTraceJob), NT_TILE, noma_trace_fill_job, false, true, false, noma_trace_launch, empty_group<prach_noma_trace, &prach_noma_trace::tx_max>, noma_trace_unpack, &prach_timing::noma_trace_ms},
    {noma_timeline_parts, sizeof(TimelineJob), TL_TILE, fill_timeline_job<true>, true, false, false, noma_timeline_launch, empty_group<prach_noma_timeline, &prach_noma_timeline::done_max>, noma_timeline_unpack, &prach_timing::noma_timeline_ms},
    {noma_gain_parts, sizeof(NomaGainJob), TL_TILE, noma_gain_fill_job, true, false, false, noma_gain_launch, empty_group<prach_noma_gain, &prach_noma_gain::level_max, &prach_noma_gain::neg_level_max>, noma_gain_unpack, &prach_timing::noma_gain_ms, noma_gain_prepass, true},
};
static_assert(sizeof(RED_KINDS) / sizeof(RED_KINDS[0]) == (size_t)Red::noma_gain + 1, "one row per kind");
const RedKind &kind_of(const Reduction &r) { return RED_KINDS[(int)r.kind]; }

// How a rerun's launch differs from the first one
struct LaunchOpts {
    bool full_calendars = false; // batch kernel: lists of nUE entries, which cannot fill (trials that filled a calendar list)
    bool host_act = false;       // NOMA.c: the activeUE table built on the host (trials whose device-built table left a gain comparison inside the error band)
    bool no_pack = false;        // no XCD-packed placement (trials of a packed launch that timed out)
};

enum class Kernel { noma, batch, lcluster, cluster, trial };
struct KernelChoice { // (rec_mode -1: noma_kernel and trial_kernel have no record layout, prach_timing keeps the previous launch's)
    Kernel kind;
    int rec_mode = -1, lslots = 0, maxgroups = 0, waves = 0, xpack = 0;
};

// the kernel, and its shape, of one launch over the trials idx[0..m) with G workgroups each (0: trial_kernel)
static KernelChoice choose_kernel(const prach_engine *e, const prach_cfg *cfgs, const int *idx, int m, int G, int maxP, LaunchOpts o) {
    const bool glibc = cfgs[idx[0]].rng_mode == PRACH_RNG_GLIBC;
    KernelChoice kc{Kernel::trial};
    if (G == 0) return kc;
    // XCD-packed launch (prach_lcluster.hip): each cluster on one XCD, eight clusters side by side — when the clusters of the launch fit
    // the XCDs' CUs that way (budgeted at one workgroup per CU: LDS-resident state fills a CU, the general layouts take more than half)
    kc.xpack = e->opt_xcd_pack && !o.no_pack && G > 1 && ((m + 7) / 8) * G <= e->num_cus / 8;
    if (cfgs[idx[0]].variant == PRACH_VARIANT_NOMA_C) { kc.kind = Kernel::noma; return kc; }
    // one workgroup per trial, Philox: the batch kernel (prach_batch.hip), within its limits
    bool batch = G == 1;
    for (int k = 0; k < m && batch; k++) batch = batch_eligible(e, cfgs[idx[k]]);
    if (batch) {
        kc.kind = Kernel::batch;
        kc.rec_mode = CLUSTER_REC_BATCH;
        // Workgroup shape (speed only, same results).  A launch is as long as its longest trial alone or as its work needs, whichever is more: a 100 000-UE
        // trial runs 127 ms on 16 wavefronts and 152 ms on 8, so while the trials fit the CUs in two rounds the 1024-thread shape wins (510 sweep trials:
        // 159 / 272 ms — Beta.c / WithNOMA — against 163 / 290 ms); past two per CU a third round starts, and two 512-thread workgroups = two trials per CU,
        // which hide each other's barriers, win (560 trials: 165 / 288 against 171 / 294 ms; 740: 171 / 327 against 218 / 395; 1000: 207 / 442 against
        // 288 / 517; 2000: 381 / 811 against 566 / 1 005): scripts/gpu_shape_probe.sh.
        kc.waves = glibc ? 16 : e->opt_batch_waves ? (int)e->opt_batch_waves : m > 2 * e->num_cus ? 8 : 16;
        return kc;
    }
    // one workgroup per trial in the reference's rand() stream: 8 + 4 byte hot records, if every subframe number of every trial of
    // the launch fits 16 bits (txTime <= t + 59 + backoff + accessTime).  (Philox with one workgroup per trial is the batch kernel's.)
    bool compact = G == 1 && !e->opt_wide_records && glibc;
    for (int k = 0; k < m && compact; k++) {
        const prach_cfg &c = cfgs[idx[k]];
        compact = (int64_t)prach_max_time(&c) + c.backoff + c.accessTime + 64 < 63000;
    }
    kc.lslots = lds_record_slots(e, cfgs, idx, m, G, maxP, &kc.maxgroups);
    kc.rec_mode = (glibc ? kc.lslots > 0 : use_fast_kernel(e, kc.lslots, maxP)) ? CLUSTER_REC_LFAST : (kc.lslots > 0 ? CLUSTER_REC_L16 : (compact ? CLUSTER_REC_H8 : CLUSTER_REC_G16));
    kc.kind = kc.rec_mode == CLUSTER_REC_LFAST ? Kernel::lcluster : Kernel::cluster;
    if (kc.rec_mode == CLUSTER_REC_H8) kc.xpack = 0;
    return kc;
}

// f(0), ..., f(n - 1) dealt round-robin to up to nth host threads (the caller's among them)
template <class F> static void parallel_for(int nth, size_t n, const F &f) {
    nth = (int)std::min<size_t>((size_t)std::max(1, nth), std::max<size_t>(1, n));
    auto work = [&](int tix) { for (size_t j = (size_t)tix; j < n; j += (size_t)nth) f(j); };
    std::vector<std::thread> th;
    for (int tix = 1; tix < nth; tix++) th.emplace_back(work, tix);
    work(0);
    for (auto &x : th) x.join();
}

// PRACH_PRINT_STAMPS (the diagnostic build's cycle stamps) and PRACH_VERBOSE (why a trial left its kernel): one trial of a finished launch
static int print_launch_diagnostics(const prach_engine *e, const prach_cfg &c, const DevResult &dr, const TrialLayout &L, const char *A, int G, bool noma) {
    if (const char *stamps = std::getenv("PRACH_PRINT_STAMPS")) {
        std::fprintf(stderr, "[prach stamps/step] pass=%.0f publish=%.0f barrier=%.0f gather=%.0f r1b=%.0f leavers=%.0f checks=%.0f grants=%.0f cycles | N avg %.1f max %llu, resetcand avg %.2f, singles avg %.1f max %llu\n",
                     dr.stamps6[0] / (double)dr.steps, dr.stamps6[1] / (double)dr.steps, dr.stamps6[2] / (double)dr.steps, dr.stamps6[3] / (double)dr.steps,
                     dr.stamps6[4] / (double)dr.steps, dr.stamps6[5] / (double)dr.steps, dr.stamps6[6] / (double)dr.steps, dr.stamps6[7] / (double)dr.steps,
                     dr.dbg[0] / (double)dr.steps, dr.dbg[1], dr.dbg[2] / (double)dr.steps, (dr.dbg[3] >> 20) / (double)dr.steps, dr.dbg[3] & 0xfffff);
        static const char *const nm[24] = {"head", "phaseB", "S1", "leavers", "S2", "publish", "window-rest", "take1", "S3", "round2", "S4", "calls", "S5", "grants", "S6", "phaseA",
                                           "w:phaseA|A-barrier", "w:loads", "w:refill", "t:buckets", "-", "-", "-", "-"};
        static const char *const nmb[24] = {"head", "joins", "-", "body", "S1", "leavers", "S2", "classify", "S4", "calls", "S5", "grants", "S6", "-", "-", "-",
                                            "-", "-", "-", "-", "-", "-", "-", "-"}; // prach_batch.hip
        static const char *const nmn[24] = {"head", "publish+gather", "gather-barrier", "resolve(w0)", "resolve-barrier", "passB+A(w0)", "pass-barrier", "-", "r:to-gains", "r:rank+sort", "r:pairing", "-", "-", "-", "-", "-",
                                            "-", "-", "-", "-", "-", "-", "-", "-"}; // prach_noma.hip, per SUBFRAME (x accessTime = per slot)
        const char *const *const names = noma ? nmn : e->last.rec_mode == CLUSTER_REC_BATCH ? nmb : nm;
        std::fprintf(stderr, "[prach fine stamps/step] nUE=%d steps=%llu", c.nUE, (unsigned long long)dr.steps);
        for (int q = 0; q < 20; q++) if (names[q][0] != '-') std::fprintf(stderr, " %s=%.0f", names[q], dr.fstamps[q] / (double)dr.steps);
        std::fprintf(stderr, "\n");
        if (L.diag && e->last.rec_mode == CLUSTER_REC_LFAST && std::atoi(stamps) >= 2) {
            // every workgroup of the cluster on its own clock (thread PRACH_STAMP_TID): cycles per subframe and phase, then its event UEs per subframe
            std::vector<unsigned long long> dg(32 * (size_t)G);
            HIPCHK(hipMemcpy(dg.data(), A + L.diag, 8 * dg.size(), hipMemcpyDeviceToHost));
            static const char *const nmw[20] = {"head", "phaseB", "S1", "leavers", "S2", "publish", "window-rest", "take1", "S3", "round2", "S4", "calls", "S5", "grants", "S6", "-",
                                                "w:phaseA", "w:loads", "w:refill", "t:buckets"};
            for (int b_ = 0; b_ < G; b_++) {
                std::fprintf(stderr, "[prach wg stamps/step] nUE=%d steps=%llu b=%d", c.nUE, (unsigned long long)dr.steps, b_);
                for (int q = 0; q < 20; q++) if (nmw[q][0] != '-') std::fprintf(stderr, " %s=%.0f", nmw[q], dg[32 * (size_t)b_ + q] / (double)dr.steps);
                std::fprintf(stderr, " queued=%.2f late-buckets=%.3f late-header=%.3f refills=%.2f\n", dg[32 * (size_t)b_ + 24] / (double)dr.steps, dg[32 * (size_t)b_ + 25] / (double)dr.steps,
                             dg[32 * (size_t)b_ + 26] / (double)dr.steps, dg[32 * (size_t)b_ + 27] / (double)dr.steps);
            }
        }
    }
    if (dr.status != PRACH_OK && e->last.rec_mode == CLUSTER_REC_LFAST && std::getenv("PRACH_VERBOSE"))
        std::fprintf(stderr, "[prach] lcluster_kernel: trial nUE=%d left at subframe %d with status %d, capacity code %d\n", c.nUE, dr.time_exit, dr.status, dr.hard_error);
    if (dr.status == PRACH_ERR_INTERNAL && e->last.rec_mode == CLUSTER_REC_BATCH && std::getenv("PRACH_VERBOSE"))
        std::fprintf(stderr, "[prach] batch_kernel: trial nUE=%d (P %d B %d G %d R %d M %d A %d u %d) left at subframe %d: capacity %d (2 reset-cycle candidates, 3 singleton callers, 4 crossing bin, 5 a join list, 6 the grant notes, 8 a chunk table, 9 the chunk pool)\n", c.nUE, c.nPreamble, c.backoff, c.nGrantUL, c.maxRarWindow, c.maxMsg2TxCount, c.accessTime, c.uniform, dr.time_exit, dr.hard_error);
    return PRACH_OK;
}

// The call's reduction over the trials `acc` that a launch finished and its caller accepts — so a trial that is rerun is counted once — behind the
// simulation kernel on the same stream; it runs while `meanwhile` turns the launch's results into prach_result on the host, and has completed on return
// (the next launch lays the arena out again and reuses the pinned job table).  Fills in every job's first workgroup; a call without a reduction only
// runs `meanwhile`.
template <class F> static int reduce_accepted(prach_engine *e, CallCtx &cx, std::vector<JobSrc> &acc, const F &meanwhile) {
    bool launched = false;
    if (cx.red) {
        const Reduction &R = *cx.red;
        const RedKind &K = kind_of(R);
        int njobs = 0, wgs = 0;
        for (JobSrc &s : acc) {
            s.wg0 = wgs;
            const int units = K.fill_job(e->red_jobs_h + K.job_bytes * (size_t)njobs++, s);
            wgs += (units + K.tile - 1) / K.tile;
            cx.trials[(size_t)s.group]++;
            cx.ues[(size_t)s.group] += (uint64_t)s.c.nUE;
        }
        if (njobs > 0 && wgs > 0) {
            HIPCHK(hipMemcpyAsync(e->red_jobs_d, e->red_jobs_h, K.job_bytes * (size_t)njobs, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipEventRecord(e->red_ev0, e->stream));
            if (K.prepass) { int rc = K.prepass(e, cx, acc, njobs, wgs); if (rc != PRACH_OK) return rc; }
            HIPCHK(K.launch(e, R, njobs, wgs, cx.d_part));
            HIPCHK(hipEventRecord(e->red_ev1, e->stream));
            launched = true;
        }
    }
    { int rc = meanwhile(); if (rc != PRACH_OK) return rc; }
    if (launched) {
        HIPCHK(hipStreamSynchronize(e->stream));
        float rms = 0;
        HIPCHK(hipEventElapsedTime(&rms, e->red_ev0, e->red_ev1));
        cx.red_ms += rms;
    }
    return PRACH_OK;
}

// one launch over the trials idx[0..m) (all the same rng_mode); attempt = glibc stream retry level.  Batch-kernel trials that filled a calendar list
// are appended to cal_overflow.
static int run_group(prach_engine *e, CallCtx &cx, const int *idx, int m, int attempt, int G, LaunchOpts o, std::vector<int> &cal_overflow) {
    const prach_cfg *const cfgs = cx.cfgs;
    const int rng_mode = cfgs[idx[0]].rng_mode;
    const bool noma = cfgs[idx[0]].variant == PRACH_VARIANT_NOMA_C;
    std::vector<size_t> slen(m, 0);
    int maxP = 1;
    for (int k = 0; k < m; k++) {
        const prach_cfg &c = cfgs[idx[k]];
        if (rng_mode == PRACH_RNG_GLIBC) slen[k] = (size_t)stream_budget(c, attempt, e->opt_stream_factor, e->draws_per_ue_seen);
        if (c.nPreamble > maxP) maxP = c.nPreamble;
    }
    const KernelChoice kc = choose_kernel(e, cfgs, idx, m, G, maxP, o);
    const bool batch = kc.kind == Kernel::batch;
    for (int k = 0; k < m; k++) // the dormant per-sector grant path exists in trial_kernel (G == 0) and in the batch kernel only
        if ((cfgs[idx[k]].flags & PRACH_FLAG_SECTOR_GRANTS) && G > 0 && !batch) return PRACH_ERR_INTERNAL;
    // NOMA.c's activeUE table: built by the device (noma_activation_kernel) unless the option or a rerun asks for the host's libm
    const bool host_act = noma && (e->opt_noma_host_activation || o.host_act);
    const LaunchLayout LL = layout_launch(cfgs, idx, m, cx.ue_logs, cx.reads_device_logs(), cx.traces(), cx.levels(), slen, G, batch, o.full_calendars, e->opt_calendar_cap);
    if (LL.end > e->mem_budget && m > 1) { // (e.g. the 10 000-trial grid with its calendars on ONE GPU: two or three launches instead of one)
        const int h = m / 2;
        int rc = run_group(e, cx, idx, h, attempt, G, o, cal_overflow);
        if (rc != PRACH_OK) return rc;
        return run_group(e, cx, idx + h, m - h, attempt, G, o, cal_overflow);
    }
    { int rc = ensure_arena(e, LL.end); if (rc != PRACH_OK) return rc; }
    { int rc = ensure_pinned(e, std::max(LL.staged_end, sizeof(DevResult) * (size_t)m)); if (rc != PRACH_OK) return rc; }
    auto t0 = std::chrono::steady_clock::now();
    char *const A = e->arena;
    char *const H = e->pinned;
    TrialDev *const td = reinterpret_cast<TrialDev *>(H);
    std::vector<int32_t> nAccess(m, 0);
    for (int k = 0; k < m; k++) {
        const prach_cfg &c = cfgs[idx[k]];
        const TrialLayout &L = LL.t[k];
        TrialDev &d = td[k];
        std::memset(&d, 0, sizeof(d));
        d.variant = c.variant; d.uniform = c.uniform; d.nUE = c.nUE; d.nP = c.nPreamble; d.backoff = c.backoff;
        d.nGrantUL = c.nGrantUL; d.maxRarWindow = c.maxRarWindow; d.maxMsg2 = c.maxMsg2TxCount; d.aT = c.accessTime;
        d.rng_mode = c.rng_mode; d.maxTime = prach_max_time(&c);
        d.stop = (c.max_steps > 0 && c.max_steps < d.maxTime) ? c.max_steps : d.maxTime;
        d.seed_lo = (unsigned)c.seed; d.seed_hi = (unsigned)(c.seed >> 32);
        d.stream_len = L.stream_len;
        d.dense_pass = e->opt_dense ? 1 : 0;
        d.pipeline = e->opt_pipeline ? 1 : 0;
        if (batch) {
            d.rec32 = reinterpret_cast<int4 *>(A + L.rec32); d.chunks = reinterpret_cast<int4 *>(A + L.chunks); d.ctab = reinterpret_cast<int *>(A + L.ctab); d.cpool = reinterpret_cast<int *>(A + L.cpool); d.nchunks = L.npool; d.tcap = L.tcap;
            d.jcal = reinterpret_cast<int *>(A + L.jcal); d.calcap = L.calcap; d.calmask = L.calslots - 1;
            d.qov = reinterpret_cast<int *>(A + L.qov); d.evov = reinterpret_cast<int2 *>(A + L.evov);
        } else {
            d.rec = reinterpret_cast<int4 *>(A + L.rec);
            d.ptc = reinterpret_cast<int *>(A + L.ptc); d.ftt = reinterpret_cast<int *>(A + L.ftt);
            d.stt = reinterpret_cast<int *>(A + L.stt); d.fcnt = reinterpret_cast<int *>(A + L.fcnt);
            d.nd = reinterpret_cast<unsigned *>(A + L.nd);
        }
        d.evbuf = L.evbuf ? reinterpret_cast<Event *>(A + L.evbuf) : nullptr;
        d.evbuf2 = L.evbuf2 ? reinterpret_cast<Event *>(A + L.evbuf2) : nullptr;
        d.sidx = L.sidx ? reinterpret_cast<int *>(A + L.sidx) : nullptr;
        d.sched = reinterpret_cast<const int *>(A + L.sched);
        d.stream = L.stream ? reinterpret_cast<const int *>(A + L.stream) : nullptr;
        d.logs = L.logs ? reinterpret_cast<prach_ue_log *>(A + L.logs) : nullptr;
        d.timers = reinterpret_cast<int *>(A + L.timers);
        d.out = reinterpret_cast<DevResult *>(A + L.out);
        d.evw = L.evw; d.mbstride = L.mbstride;
        d.binshift = 0;
        while (((c.nUE - 1) >> d.binshift) >= 1024) d.binshift++;
        d.mbox = L.mbox ? reinterpret_cast<int *>(A + L.mbox) : nullptr;
        d.cand = L.cand ? reinterpret_cast<int2 *>(A + L.cand) : nullptr;
        d.flags = c.flags;
        d.diag = L.diag ? reinterpret_cast<unsigned long long *>(A + L.diag) : nullptr;
        d.sector = L.sector ? reinterpret_cast<int *>(A + L.sector) : nullptr;
        d.trace = L.trace ? reinterpret_cast<int4 *>(A + L.trace) : nullptr;
        int32_t *sched = reinterpret_cast<int32_t *>(H + L.sched);
        // the arrival table depends on (nUE, traffic law, accessTime) only: a sweep x seeds batch has a handful of distinct ones
        // (2000 pow() calls each) — copy the previous trial's table when its key is the same
        int same = -1;
        for (int q = k - 1; q >= 0 && q >= k - 16; q--) {
            const prach_cfg &o = cfgs[idx[q]];
            if (o.nUE == c.nUE && o.uniform == c.uniform && o.accessTime == c.accessTime && o.variant == c.variant) { same = q; break; }
        }
        if (same >= 0) {
            std::memcpy(sched, H + LL.t[same].sched, 4 * L.sched_len);
            nAccess[k] = nAccess[same];
        } else {
            for (size_t s = 0; s < L.sched_len; s++) sched[s] = c.nUE;
            prach_arrival_schedule(&c, sched, (int)L.sched_len, &nAccess[k]);
        }
        if (rng_mode == PRACH_RNG_GLIBC)
            // the reference's rand() stream window [stream_offset, +stream_len): the host only jumps ahead (31-word window
            // per chunk, cached matrix powers); the values themselves are generated on the device inside the timed region
            reinterpret_cast<StreamJob *>(H + LL.stream_jobs)[k] = StreamJob{reinterpret_cast<const unsigned *>(A + L.seeds), reinterpret_cast<int *>(A + L.stream), (unsigned long long)L.stream_len};
        if (noma) {
            d.n_pre0 = reinterpret_cast<const int *>(A + L.n_pre0); d.n_sector = reinterpret_cast<const int *>(A + L.n_sector);
            d.n_gain = reinterpret_cast<const double *>(A + L.n_gain); d.n_lgain = reinterpret_cast<const double *>(A + L.n_lgain);
            d.n_nd0 = reinterpret_cast<const unsigned *>(A + L.n_nd0);
            d.cell_radius = c.cellRadius;
            d.n_devact = host_act ? 0 : (e->opt_noma_ambiguity_test ? 2 : 1);
        }
    }
    if (rng_mode == PRACH_RNG_GLIBC) // one 31-word window per chunk of every trial's stream window: the trials dealt to the host cores (100 trials x 200 jump-aheads: 25 ms on one)
        parallel_for(host_threads(e), (size_t)m, [&](size_t k) {
            const prach_cfg &c = cfgs[idx[k]];
            const TrialLayout &L = LL.t[k];
            prach_internal_glibc_seeds((uint32_t)c.seed, c.stream_offset, L.nchunks, STREAM_CHUNK, reinterpret_cast<uint32_t *>(H + L.seeds));
        });
    if (noma && host_act) {
        // activeUE's per-UE attributes (NOMA.c:131-192: double-precision libm work, once per UE): built on the host with the
        // libm the reference links, UE ranges of all trials dealt to all host cores, then copied trial by trial
        const int nth = host_threads(e);
        struct Tab { std::vector<int32_t> pre0, sec; std::vector<double> gn, lg; std::vector<uint32_t> nd0; };
        std::vector<Tab> tabs(m);
        struct Job { int k, lo, hi; };
        std::vector<Job> jobs;
        for (int k = 0; k < m; k++) {
            const int n = cfgs[idx[k]].nUE;
            tabs[k].pre0.resize(n); tabs[k].sec.resize(n); tabs[k].gn.resize(n); tabs[k].lg.resize(n); tabs[k].nd0.resize(n);
            const int step = std::max(2048, (n + nth - 1) / nth);
            for (int lo = 0; lo < n; lo += step) jobs.push_back({k, lo, std::min(n, lo + step)});
        }
        std::vector<int> jrc(jobs.size(), PRACH_OK);
        parallel_for(nth, jobs.size(), [&](size_t j) {
            const Job &J = jobs[j];
            Tab &T = tabs[J.k];
            jrc[j] = prach_noma_activation_range(&cfgs[idx[J.k]], J.lo, J.hi, T.pre0.data() + J.lo, T.sec.data() + J.lo, T.gn.data() + J.lo,
                                                 T.lg.data() + J.lo, T.nd0.data() + J.lo);
        });
        for (int r : jrc) if (r != PRACH_OK) return r;
        for (int k = 0; k < m; k++) {
            const size_t nn = (size_t)cfgs[idx[k]].nUE;
            const TrialLayout &L = LL.t[k];
            HIPCHK(hipMemcpyAsync(A + L.n_pre0, tabs[k].pre0.data(), 4 * nn, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(A + L.n_sector, tabs[k].sec.data(), 4 * nn, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(A + L.n_gain, tabs[k].gn.data(), 8 * nn, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(A + L.n_lgain, tabs[k].lg.data(), 8 * nn, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(A + L.n_nd0, tabs[k].nd0.data(), 4 * nn, hipMemcpyHostToDevice, e->stream));
        }
        HIPCHK(hipStreamSynchronize(e->stream)); // (the tables are pageable host memory that goes away)
    }
    // ONE copy stages every parameter block, arrival table and stream seed of the launch; ONE memset zeroes everything the
    // kernels accumulate into or poll (DevResult blocks; mailbox tags: 0 never equals t + 1)
    HIPCHK(hipMemcpyAsync(A, H, LL.staged_end, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(A + LL.zero_begin, 0, LL.zero_end - LL.zero_begin, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    auto t1 = std::chrono::steady_clock::now();
    cx.upload_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();

    const TrialDev *const dp = reinterpret_cast<const TrialDev *>(A);
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    if (rng_mode == PRACH_RNG_GLIBC) { // every trial's stream window, ONE launch (a launch per trial: 0.45 ms each, prach_stream.hip)
        unsigned long long max_n = 0;
        for (int k = 0; k < m; k++) max_n = std::max(max_n, (unsigned long long)LL.t[k].stream_len);
        HIPCHK(launch_glibc_stream_jobs(reinterpret_cast<const StreamJob *>(A + LL.stream_jobs), m, max_n, e->stream));
    }
    if (noma && !host_act) { // activeUE for every UE of the launch, inside the timed region
        std::vector<ActTab> tabs(m);
        for (int k = 0; k < m; k++) tabs[k] = {A + LL.t[k].n_pre0, A + LL.t[k].n_sector, A + LL.t[k].n_gain, A + LL.t[k].n_lgain, A + LL.t[k].n_nd0};
        int rc = noma_device_activation(e, dp, cfgs, idx, m, tabs, reinterpret_cast<unsigned *>(A + LL.act_flags), nullptr, cx.noma_flagged);
        if (rc == NOMA_ACT_OVERFLOW_RC) { // the same launch once more with the host-built table (the path a NOMA_AMBIGUOUS rerun takes)
            o.host_act = true;
            return run_group(e, cx, idx, m, attempt, G, o, cal_overflow);
        }
        if (rc != PRACH_OK) return rc;
    }
    const bool glibc = rng_mode == PRACH_RNG_GLIBC;
    switch (kc.kind) {
    case Kernel::noma: HIPCHK(launch_noma_kernel(dp, m, G, maxP, kc.xpack, e->stream)); break;
    case Kernel::batch: HIPCHK(launch_batch_kernel(dp, m, kc.waves, glibc, e->stream)); break;
    case Kernel::lcluster: HIPCHK(launch_lcluster_kernel(dp, m, G, kc.lslots, kc.xpack, glibc, kc.maxgroups, e->stream)); break;
    case Kernel::cluster: HIPCHK(launch_cluster_kernel(dp, m, G, maxP, rng_mode, kc.rec_mode, kc.lslots, kc.xpack, e->stream)); break;
    case Kernel::trial: HIPCHK(launch_trial_kernel(dp, m, rng_mode, maxP, e->stream)); break;
    }
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipMemcpyAsync(H, A + LL.out0, sizeof(DevResult) * (size_t)m, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    cx.kernel_ms += ms;
    e->last.launches++;
    e->last.workgroups = m * (G > 0 ? G : 1);
    e->last.cluster_size = G;
    if (kc.kind != Kernel::trial) e->last.xcd_packed = kc.xpack; // (trial_kernel has no placement: prach_timing keeps the previous launch's)
    if (kc.rec_mode >= 0) e->last.rec_mode = kc.rec_mode;

    const DevResult *const drs = reinterpret_cast<const DevResult *>(H);
    // the call's reduction over the trials the loop below accepts: dist reads the timers and preamble counts the simulation kernel left in the arena,
    // timeline and sojourn its log records and the launch's own copy of every arrival schedule
    std::vector<JobSrc> acc;
    for (int k = 0; k < m && cx.red; k++)
        if (drs[k].status == PRACH_OK && !(noma && drs[k].hard_error == NOMA_AMBIGUOUS)) acc.push_back(JobSrc{cfgs[idx[k]], LL.t[k], drs[k], A, cx.group_of(idx[k]), 0, batch});
    return reduce_accepted(e, cx, acc, [&]() -> int {
        std::vector<int32_t> timers;
        for (int k = 0; k < m; k++) {
            const prach_cfg &c = cfgs[idx[k]];
            const TrialLayout &L = LL.t[k];
            const DevResult &dr = drs[k];
            prach_result &r = cx.results[idx[k]];
            std::memset(&r, 0, sizeof(r));
            r.status = (dr.hard_error && dr.status == PRACH_ERR_TIMEOUT) ? PRACH_ERR_INTERNAL : dr.status; // (a capacity overflow somewhere in the cluster is the cause, a peer's time-out its effect)
            if (noma && dr.hard_error == NOMA_AMBIGUOUS && r.status == PRACH_OK) { r.status = PRACH_ERR_INTERNAL; cx.noma_ambiguous++; } // (rerun with the host-built table: run_trials)
            r.time_exit = dr.time_exit;
            r.maxTime = prach_max_time(&c);
            r.nSuccessUE = dr.nSuccess;
            r.failedUEs = c.nUE - dr.nSuccess;
            r.preambleTxCount = dr.ptcSum;
            r.failCounts = dr.fcSum;
            r.collisionPreambles = dr.collisionPreambles;
            r.totalPreambleTxop = dr.totalPreambleTxop;
            r.activeCheck = dr.activeCheck;
            r.nAccessUE = nAccess[k];
            r.continueFaliedUEs = dr.continueFailed;
            r.finalSuccessUEs = dr.finalSuccess;
            r.sumTimer = dr.sumTimer;
            r.draws = dr.draws;
            r.steps = steps_of(c, dr);
            e->last.group_visits += dr.visits;
            e->last.event_ues += dr.events;
            if (c.variant == PRACH_VARIANT_NOMA_C && dr.nSuccess == c.nUE && dr.dbg[0] > 0) { // all UEs succeeded: NOMA.c:707-710 breaks there
                r.time_exit = (int32_t)dr.dbg[0] - 1; // (r.steps: steps_of above)
            }
            { int rc = print_launch_diagnostics(e, c, dr, L, A, G, noma); if (rc != PRACH_OK) return rc; }
            if (batch && dr.status == PRACH_ERR_INTERNAL && (dr.hard_error == 5 || dr.hard_error == 8 || dr.hard_error == 9) && !o.full_calendars) cal_overflow.push_back(idx[k]);
            if (dr.status != PRACH_OK) continue;
            // totalDelay is a FLOAT running sum in index order (Beta.c:186,193): exact in integer
            // arithmetic while it stays below 2^24, otherwise replay the float additions on the host.
            if (dr.sumTimer < (1ll << 24)) {
                r.totalDelay = (float)dr.sumTimer;
            } else {
                timers.resize((size_t)c.nUE);
                HIPCHK(hipMemcpy(timers.data(), A + L.timers, 4 * (size_t)c.nUE, hipMemcpyDeviceToHost));
                float td_ = 0;
                for (int i = 0; i < c.nUE; i++)
                    if (timers[i] != INT_MIN) td_ += (float)timers[i];
                r.totalDelay = td_;
            }
            if (L.logs && cx.ue_logs && cx.ue_logs[idx[k]]) // (a timeline call lays out every trial's log; only the ones asked for cross the bus)
                HIPCHK(hipMemcpy(cx.ue_logs[idx[k]], A + L.logs, sizeof(prach_ue_log) * (size_t)c.nUE, hipMemcpyDeviceToHost));
        }
        return PRACH_OK;
    });
}

// A trial that a cluster launch could not finish — a per-subframe LDS capacity exceeded (PRACH_ERR_INTERNAL) or a workgroup
// that waited too long for a peer (PRACH_ERR_TIMEOUT: the cluster's workgroups were not all resident, e.g. another process
// holds CUs) — is rerun, exactly, on a kernel that needs neither.  Never silently: counted in prach_timing and reported.
static void note_fallback(prach_engine *e, const CallCtx &cx, const char *what, const std::vector<int> &trials, int G) {
    const size_t ntrials = trials.size();
    size_t ntimeouts = 0;
    for (int k : trials) ntimeouts += cx.results[k].status == PRACH_ERR_TIMEOUT;
    e->last.fallback_trials += (int32_t)ntrials;
    e->last.spin_timeouts += (int32_t)ntimeouts;
    std::fprintf(stderr, "[prach] %zu trial(s) of a %d-workgroup cluster launch are rerun on %s (%zu exceeded a per-subframe capacity, %zu timed out "
                         "waiting for a peer workgroup: cluster not co-resident?)\n", ntrials, G, what, ntrials - ntimeouts, ntimeouts);
}

// The trials `todo` with G workgroups each (0: trial_kernel) until each has finished or left its kernel: a trial whose glibc draw-stream window ran out
// is rerun with a larger one (attempt + 1; after 7 attempts: PRACH_ERR_STREAM); batch-kernel trials that filled a calendar list (a parameter set that
// synchronises more UEs onto one subframe than the list was sized for) once more with lists of nUE entries, which cannot fill — never silently: counted
// as fallback trials and reported; with `unpack`, trials that timed out on an XCD-packed launch at attempt + 1 as a plain one (not a fallback either).
// `left`: the trials that ended in PRACH_ERR_INTERNAL or PRACH_ERR_TIMEOUT.
static int run_with_retries(prach_engine *e, CallCtx &cx, std::vector<int> todo, int G, LaunchOpts o, std::vector<int> *left = nullptr, bool unpack = false) {
    if (left) left->clear();
    for (int attempt = 0; !todo.empty(); attempt++) {
        if (attempt > 6) return PRACH_ERR_STREAM;
        std::vector<int> cal, again;
        int rc = run_group(e, cx, todo.data(), (int)todo.size(), attempt, G, o, cal);
        if (rc != PRACH_OK) return rc;
        if (!cal.empty()) {
            e->last.fallback_trials += (int32_t)cal.size();
            std::fprintf(stderr, "[prach] %zu trial(s) filled a calendar list of prach::batch_kernel: rerun with lists of nUE entries\n", cal.size());
            LaunchOpts full = o;
            full.full_calendars = true;
            rc = run_with_retries(e, cx, cal, G, full); // (these trials are in `todo` as well: their statuses are read below)
            if (rc != PRACH_OK) return rc;
        }
        const bool was_packed = e->last.xcd_packed != 0;
        o.no_pack = false;
        for (int k : todo) {
            const int s = cx.results[k].status;
            if (s == PRACH_ERR_STREAM) again.push_back(k); // (the reference's stream: a larger window)
            else if (s == PRACH_ERR_TIMEOUT && was_packed && unpack) { // the packed placement did not hold: plain cluster launch
                again.push_back(k);
                o.no_pack = true;
            }
            else if ((s == PRACH_ERR_INTERNAL || s == PRACH_ERR_TIMEOUT) && left) left->push_back(k);
        }
        if (o.no_pack) {
            std::fprintf(stderr, "[prach] %zu trial(s) of an XCD-packed cluster launch timed out waiting for a peer workgroup: rerun as a plain cluster launch\n", again.size());
            e->last.spin_timeouts += (int32_t)again.size();
        }
        todo.swap(again);
    }
    return PRACH_OK;
}

// ---- NOMA.c in the reference's OWN rand() stream (prach_noma_glibc.hip): activeUE's rejection loops make every stream position data dependent and its
// libm calls must be the reference's — the bit-exact-vs-the-reference's-files mode, not the throughput mode.  Both forms lie in the arena like any launch.

// The slot-by-slot form between the engine's two events: one launch per access slot, the slot's arrivals activated by the host between two launches with the
// libm the reference links, from the host's copy `hs` of the window; the finishing kernel behind the last slot.  PRACH_ERR_STREAM: the window ran out.
static int noma_glibc_slot_loop(prach_engine *e, const prach_cfg &c, const NomaGlibcLayout &L, const int32_t *hs) {
    char *const A = e->arena, *const H = e->pinned;
    const size_t ue = L.t[0].ue, ue_bytes = L.ue_bytes;
    const int32_t *const sched = reinterpret_cast<const int32_t *>(H + L.t[0].sched);
    uint64_t pos = 0;
    for (int s = 0, t = 0, activeCheck = 0;; s++, t += c.accessTime) {
        const int prevAC = activeCheck;
        activeCheck = sched[s]; // NOMA.c:675-681
        int rc = noma_glibc_stage_slot(L, c, hs, &pos, t, prevAC, activeCheck, H);
        if (rc != PRACH_OK) return rc;
        if (activeCheck > prevAC)
            HIPCHK(hipMemcpyAsync(A + ue + ue_bytes * (size_t)prevAC, H + ue + ue_bytes * (size_t)prevAC, ue_bytes * (size_t)(activeCheck - prevAC), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(A + L.ctl, H + L.ctl, L.ctl_bytes, hipMemcpyHostToDevice, e->stream));
        HIPCHK(launch_noma_glibc_slot(L, c, A, e->stream));
        HIPCHK(hipMemcpyAsync(H + L.ctl, A + L.ctl, L.ctl_bytes, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        const NomaGlibcEnd end = noma_glibc_end(L, c, H, 0);
        if (end.status != PRACH_OK) return end.status;
        pos = end.pos;
        if (end.done) break;
    }
    HIPCHK(launch_noma_glibc_finish(L, A, e->stream));
    return PRACH_OK;
}

// One launch over the trials idx[0..m) with the windows lens[]: the single-launch form (side by side, one workgroup each, activeUE on the device) or,
// `slots`, one trial slot by slot.  A trial whose window ran out is appended to `again`; one with a value inside the device math library's error band
// (prach_noma_act.h: a few percent of the trials) to `ambiguous`.  The others are finished: prach_result (saveResult, NOMA.c:618-625) from the control
// blocks, the logs that were asked for straight from the arena, the call's reduction over what the finishing kernel left there.
static int noma_glibc_launch(prach_engine *e, CallCtx &cx, const int *idx, int m, const unsigned long long *lens, bool slots, std::vector<int> &again, std::vector<int> &ambiguous) {
    const NomaGlibcLayout L = noma_glibc_layout(cx.cfgs, idx, m, lens, cx.ue_logs, slots);
    if (L.end > e->mem_budget && m > 1) { // (as run_group: several launches instead of one; one trial alone always runs)
        int rc = noma_glibc_launch(e, cx, idx, m / 2, lens, slots, again, ambiguous);
        return rc != PRACH_OK ? rc : noma_glibc_launch(e, cx, idx + m / 2, m - m / 2, lens + m / 2, slots, again, ambiguous);
    }
    { int rc = ensure_arena(e, L.end); if (rc != PRACH_OK) return rc; }
    { int rc = ensure_pinned(e, L.staged_end); if (rc != PRACH_OK) return rc; }
    char *const A = e->arena, *const H = e->pinned;
    std::vector<int32_t> nAccess((size_t)m, 0), hs; // hs: the slot form's host copy of the window
    if (slots) { hs.resize((size_t)lens[0]); prach_glibc_stream((uint32_t)cx.cfgs[idx[0]].seed, cx.cfgs[idx[0]].stream_offset, lens[0], hs.data()); }
    noma_glibc_stage(L, cx.cfgs, idx, A, H, nAccess.data());
    e->last.launches++;
    HIPCHK(hipMemcpyAsync(A, H, L.staged_end, hipMemcpyHostToDevice, e->stream));
    if (slots) HIPCHK(hipMemcpyAsync(A + L.t[0].stream, hs.data(), 4 * hs.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipEventRecord(e->ev0, e->stream));
    if (slots) {
        int rc = noma_glibc_slot_loop(e, cx.cfgs[idx[0]], L, hs.data());
        if (rc == PRACH_ERR_STREAM) { again.push_back(idx[0]); return PRACH_OK; }
        if (rc != PRACH_OK) return rc;
    } else HIPCHK(launch_noma_glibc_trials(L, A, e->stream));
    HIPCHK(hipEventRecord(e->ev1, e->stream));
    HIPCHK(hipMemcpyAsync(H + L.ctl, A + L.ctl, L.ctl_bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    cx.kernel_ms += ms;
    static const DevResult no_result{};
    std::vector<TrialLayout> tl((size_t)m, TrialLayout{});
    std::vector<JobSrc> acc;
    std::vector<int> ok;
    for (int j = 0; j < m; j++) {
        const int st = noma_glibc_end(L, cx.cfgs[idx[j]], H, j).status;
        if (st == PRACH_ERR_STREAM) again.push_back(idx[j]);
        else if (st == NOMA_GLIBC_AMBIGUOUS_RC) ambiguous.push_back(idx[j]);
        else if (st != PRACH_OK) return st;
        else {
            ok.push_back(j);
            tl[j].timers = L.t[j].timers; tl[j].ptc = L.t[j].ptc; // (all that dist_fill_job reads)
            if (cx.red) acc.push_back(JobSrc{cx.cfgs[idx[j]], tl[j], no_result, A, cx.group_of(idx[j]), 0, false});
        }
    }
    return reduce_accepted(e, cx, acc, [&]() -> int {
        for (int j : ok) {
            const prach_cfg &c = cx.cfgs[idx[j]];
            const NomaGlibcEnd t = noma_glibc_end(L, c, H, j);
            prach_result &r = cx.results[idx[j]];
            std::memset(&r, 0, sizeof(r));
            r.status = PRACH_OK; r.time_exit = t.time_exit; r.maxTime = 10000; r.steps = t.steps; r.draws = t.pos;
            r.nSuccessUE = r.finalSuccessUEs = t.nSuccess; r.failedUEs = c.nUE - t.nSuccess; r.activeCheck = t.activeCheck; r.nAccessUE = nAccess[j];
            r.preambleTxCount = t.nTxP; r.failCounts = t.failed; r.sumTimer = t.delay; r.totalDelay = (float)t.delay;
            if (L.t[j].logs) HIPCHK(hipMemcpy(cx.ue_logs[idx[j]], A + L.t[j].logs, sizeof(prach_ue_log) * (size_t)c.nUE, hipMemcpyDeviceToHost));
        }
        return PRACH_OK;
    });
}

// The NOMA.c trials `todo` of a call in the reference's stream: the single-launch form, then slot by slot what it handed on.  The window of a trial, in
// either form, is 48, 192, 768, 3072 values per UE (1.2 GB at nUE = 100 000 at most); a trial that has used up the fourth ends the call with PRACH_ERR_STREAM.
static int run_noma_glibc(prach_engine *e, CallCtx &cx, std::vector<int> todo) {
    std::vector<int> ambiguous;
    if (e->opt_noma_ambiguity_test && !e->opt_noma_host_activation) ambiguous.swap(todo); // (test hook: as if the kernel had found a value inside the band in every trial)
    for (const bool slots : {e->opt_noma_host_activation != 0, true}) {
        for (int attempt = 0; !todo.empty(); attempt++) {
            if (attempt >= 4) return PRACH_ERR_STREAM;
            std::vector<unsigned long long> lens;
            for (int k : todo) lens.push_back(((unsigned long long)cx.cfgs[k].nUE * 48ull + (1ull << 18)) << (2 * attempt));
            std::vector<int> again;
            const int m = (int)todo.size(), per = slots ? 1 : m; // (slot by slot: one trial at a time)
            for (int j = 0; j < m; j += per) {
                int rc = noma_glibc_launch(e, cx, todo.data() + j, per, lens.data() + j, slots, again, ambiguous);
                if (rc != PRACH_OK) return rc;
            }
            todo.swap(again);
        }
        for (int k : ambiguous) {
            cx.noma_ambiguous++;
            e->last.fallback_trials++;
            if (std::getenv("PRACH_VERBOSE")) std::fprintf(stderr, "[prach] NOMA.c trial nUE=%d in the reference's stream: a value inside the device libm's error band, rerun with host-side activation\n", cx.cfgs[k].nUE);
        }
        todo.swap(ambiguous);
        ambiguous.clear();
    }
    return PRACH_OK;
}

// The fallback ladder of Beta.c / WithNOMA trials, cluster(G) -> prach::batch_kernel -> trial_kernel, entered at cluster(G) (G = 1 on batch-eligible
// trials: the batch kernel itself).  What is left for trial_kernel is appended to `to_trial`, which the caller runs with the trials that start there.
static int descend_ladder(prach_engine *e, CallCtx &cx, const std::vector<int> &idx, int G, std::vector<int> &to_trial) {
    std::vector<int> left;
    int rc = run_with_retries(e, cx, idx, G, LaunchOpts{}, &left, true);
    if (rc != PRACH_OK) return rc;
    if (left.empty()) return PRACH_OK;
    bool to_batch = G > 1;
    for (int k : left) to_batch = to_batch && batch_eligible(e, cx.cfgs[k]);
    note_fallback(e, cx, to_batch ? "prach::batch_kernel (one workgroup per trial, event queue without a capacity)"
                                  : "trial_kernel (one workgroup per trial, no per-subframe capacity)", left, G);
    if (to_batch) {
        // Overflow without the cliff: most capacities a cluster trips over are PER WORKGROUP (512 event granules per mailbox, the
        // candidate list) or come with its LDS-resident layout; prach::batch_kernel has neither (one workgroup, the event queue
        // continues in global memory) and still runs all 16 wavefronts on the trial, so such trials go there first — the
        // one-workgroup, index-ordered trial_kernel (no per-subframe capacity at all, ~10x slower) only gets what is left.
        std::vector<int> still;
        rc = run_with_retries(e, cx, left, 1, LaunchOpts{}, &still);
        if (rc != PRACH_OK) return rc;
        left.swap(still);
        if (!left.empty()) std::fprintf(stderr, "[prach] %zu of them exceeded a capacity of the batch kernel's resolver too: rerun on trial_kernel\n", left.size());
    }
    e->last.trial_kernel_reruns += (int32_t)left.size();
    to_trial.insert(to_trial.end(), left.begin(), left.end());
    return PRACH_OK;
}

// Workgroups per trial of a cluster launch over the trials idx: the engine option, or else the largest power of two up to `cap` that fits the resident
// workgroups and leaves each workgroup 16 UE groups or more (`overrides`: then the measured exceptions); last, halved until every cluster is resident.
static int cluster_size(const prach_engine *e, const prach_cfg *cfgs, const std::vector<int> &idx, size_t resident, int cap, bool overrides) {
    int minGroups = INT_MAX;
    for (int k : idx) minGroups = std::min(minGroups, (cfgs[k].nUE + 63) / 64);
    int G = (int)e->opt_cluster;
    if (G <= 0) {
        G = 1;
        while (G * 2 <= cap && (size_t)G * 2 * idx.size() <= resident && G * 2 <= std::max(1, minGroups / 16)) G *= 2;
        if (overrides) {
            bool all_batch = true;
            for (int k : idx) all_batch = all_batch && batch_eligible(e, cfgs[k]);
            // two workgroups per trial are not worth their exchange: 100 sweep trials run 151 / 242 ms (Beta.c / WithNOMA) on the batch kernel, one
            // workgroup each, against 221 / 471 ms on 2-workgroup clusters, whose halves of a 100 000-UE trial also overflow the 512 event
            // granules of a mailbox (32 of 100 trials rerun); from four workgroups per trial on, clusters win (scripts/gpu_probe_mid_batches.py)
            // (the reference's own stream, 100 trials of one sweep point: 246 / 431 ms on batch_kernel<16, true> against 657 / 2 126 ms — Beta.c / WithNOMA,
            //  nUE = 100 000, the latter with every trial overflowing its mailboxes — on 2-workgroup clusters: scripts/gpu_probe_glibc_batches.py)
            // (in the reference's stream also against four workgroups per trial, which run on the general kernel: 50 trials 210 / 338 ms against 351 / 501 ms
            //  at nUE = 100 000, 73 / 100 against 84 / 108 ms at 20 000; from eight workgroups per trial on the clusters are level or ahead)
            // (round 4's batch kernel is level with four workgroups per trial in Philox mode as well: 60 sweep trials 126 / 185 ms — Beta.c / WithNOMA — against
            //  136 / 190 ms on 4-workgroup clusters; eight workgroups per trial stay ahead: 30 trials 95 / 118 against 126 / 184 ms)
            if ((G == 2 || G == 4) && all_batch) G = 1;
            // Uniform arrivals over 60 000 subframes (Beta.c:92-95): only nUE / 60 000 arrivals per subframe, a UE lives some
            // tens of subframes, finished groups are skipped 32 at a time — the live band is a few groups and one workgroup
            // steps through a subframe faster than a cluster exchanges (nUE = 100 000: 5.1 vs 6.2 us per subframe)
            bool light = cfgs[idx[0]].rng_mode == PRACH_RNG_PHILOX;
            for (int k : idx) light = light && cfgs[k].uniform && cfgs[k].nUE <= 2000000;
            if (light) G = 1;
        }
    }
    while (G > 1 && (size_t)G * idx.size() > resident) G /= 2;
    return G;
}

// grows the call's device buffer and the job table of a launch (n: the most trials one launch can hold), carves the buffer into its parts and zeroes it on
// the engine's stream
static int reduction_begin(prach_engine *e, CallCtx &cx, int n) {
    const Reduction &R = *cx.red;
    const RedKind &K = kind_of(R);
    const size_t ng = (size_t)R.ngroups;
    size_t words[RED_MAX_PARTS], at[RED_MAX_PARTS], need = 0;
    const int np = K.parts(R, words);
    for (int q = 0; q < np; q++) { at[q] = align_up(need, 256); need = at[q] + 8 * ng * words[q]; }
    const size_t at_table = align_up(need, 256);
    if (R.table_bytes) need = at_table + R.table_bytes;
    if (need > e->red_cap) {
        if (e->red_buf) HIPCHK(hipFree(e->red_buf));
        e->red_buf = nullptr; e->red_cap = 0;
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&e->red_buf), need));
        e->red_cap = need;
    }
    if (K.job_bytes * (size_t)n > e->red_jobs_cap) {
        if (e->red_jobs_h) HIPCHK(hipHostFree(e->red_jobs_h));
        if (e->red_jobs_d) HIPCHK(hipFree(e->red_jobs_d));
        e->red_jobs_h = e->red_jobs_d = nullptr; e->red_jobs_cap = 0;
        const size_t want = K.job_bytes * (size_t)(n + (n >> 2) + 64);
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&e->red_jobs_h), want, hipHostMallocDefault));
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&e->red_jobs_d), want));
        e->red_jobs_cap = want;
    }
    if (!e->red_ev0) HIPCHK(hipEventCreate(&e->red_ev0));
    if (!e->red_ev1) HIPCHK(hipEventCreate(&e->red_ev1));
    for (int q = 0; q < np; q++) cx.d_part[q] = reinterpret_cast<unsigned long long *>(e->red_buf + at[q]);
    cx.trials.assign(ng, 0);
    cx.ues.assign(ng, 0);
    HIPCHK(hipMemsetAsync(e->red_buf, 0, need, e->stream));
    e->red_table = R.table_bytes ? e->red_buf + at_table : nullptr;
    if (R.table_bytes) HIPCHK(hipMemcpyAsync(e->red_buf + at_table, R.table, R.table_bytes, hipMemcpyHostToDevice, e->stream));
    e->red_bulk = nullptr; e->red_bulk_pitch = 0;
    if (R.bulk_width) { // the bulk part: the engine's own buffer, rows without gaps, or the caller's device memory; ONE fill on the engine's stream
        const size_t bytes = R.bulk_width * R.bulk_rows;
        if (!R.bulk_dev && bytes > e->bulk_cap) {
            if (e->bulk_buf) HIPCHK(hipFree(e->bulk_buf));
            e->bulk_buf = nullptr; e->bulk_cap = 0;
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&e->bulk_buf), bytes));
            e->bulk_cap = bytes;
        }
        e->red_bulk = R.bulk_dev ? static_cast<char *>(R.bulk_dev) : e->bulk_buf;
        e->red_bulk_pitch = R.bulk_dev ? R.bulk_pitch : R.bulk_width;
        if (e->red_bulk_pitch == R.bulk_width || R.bulk_rows == 1) HIPCHK(hipMemsetAsync(e->red_bulk, R.bulk_fill, bytes, e->stream));
        else HIPCHK(hipMemset2DAsync(e->red_bulk, e->red_bulk_pitch, R.bulk_fill, R.bulk_width, R.bulk_rows, e->stream));
    }
    return PRACH_OK;
}
// ONE copy-out per part at the end of the call (every reduction kernel has completed: run_group waits for its own); the scalars are unpacked group by
// group by the kind; the last failure is the call's
static int reduction_end(prach_engine *e, CallCtx &cx) {
    const Reduction &R = *cx.red;
    const RedKind &K = kind_of(R);
    const size_t ng = (size_t)R.ngroups;
    size_t words[RED_MAX_PARTS];
    const int np = K.parts(R, words);
    const size_t nsc = words[np - 1];
    std::vector<unsigned long long> sc(ng * nsc);
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int q = 0; q + 1 < np; q++) HIPCHK(hipMemcpy(R.out[q], cx.d_part[q], 8 * ng * words[q], hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sc.data(), cx.d_part[np - 1], 8 * sc.size(), hipMemcpyDeviceToHost));
    if (R.bulk_width && !R.bulk_dev) { // the engine's copy of the bulk part, once
        if (R.bulk_pitch == R.bulk_width || R.bulk_rows == 1) HIPCHK(hipMemcpy(R.bulk_host, e->red_bulk, R.bulk_width * R.bulk_rows, hipMemcpyDeviceToHost));
        else HIPCHK(hipMemcpy2D(R.bulk_host, R.bulk_pitch, e->red_bulk, R.bulk_width, R.bulk_width, R.bulk_rows, hipMemcpyDeviceToHost));
    }
    int rc = PRACH_OK;
    for (size_t g = 0; g < ng; g++) {
        const int grc = K.unpack(R, cx, g, &sc[g * nsc]);
        if (grc != PRACH_OK) rc = grc;
    }
    return rc;
}

static int run_trials_impl(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const Reduction *red = nullptr) {
    for (int k = 0; k < n; k++) { // nothing is left uninitialised on an early error return
        std::memset(&results[k], 0, sizeof(results[k]));
        results[k].status = PRACH_ERR_INTERNAL;
    }
    if (red) { // (the same for the reduction's outputs: empty groups)
        const size_t ng = (size_t)red->ngroups;
        size_t words[RED_MAX_PARTS];
        const int np = kind_of(*red).parts(*red, words);
        for (int q = 0; q + 1 < np; q++) std::memset(red->out[q], 0, 8 * ng * words[q]);
        for (size_t g = 0; g < ng; g++) kind_of(*red).empty(*red, g, cfgs);
    }
    for (int k = 0; k < n; k++) {
        int v = prach_cfg_validate(&cfgs[k]);
        if (v != PRACH_OK) return v;
        if (cfgs[k].variant == PRACH_VARIANT_NOMA_C && (cfgs[k].nPreamble > 64 || cfgs[k].uniform)) return PRACH_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(e->device));
    auto t0 = std::chrono::steady_clock::now();
    e->last = prach_timing{};
    CallCtx cx{cfgs, results, ue_logs};
    // (a trace call takes the paths that "fast" = 0 takes)
    struct FastOff { prach_engine *e; int64_t was; ~FastOff() { e->opt_fast = was; } } fast_off{e, e->opt_fast};
    if (red && kind_of(*red).fast_off) e->opt_fast = 0;
    if (red) {
        cx.red = red;
        int rc = reduction_begin(e, cx, n);
        if (rc != PRACH_OK) return rc;
    }
    { // NOMA.c in the reference's OWN rand() stream (prach_noma_glibc.hip)
        std::vector<int> idx;
        for (int k = 0; k < n; k++)
            if (cfgs[k].variant == PRACH_VARIANT_NOMA_C && cfgs[k].rng_mode == PRACH_RNG_GLIBC) idx.push_back(k);
        int rc = run_noma_glibc(e, cx, idx);
        if (rc != PRACH_OK) return rc;
    }
    { // NOMA.c variant (Philox): its own kernel, G workgroups per trial like the production kernel
        std::vector<int> idx;
        for (int k = 0; k < n; k++)
            if (cfgs[k].variant == PRACH_VARIANT_NOMA_C && cfgs[k].rng_mode == PRACH_RNG_PHILOX) idx.push_back(k);
        if (!idx.empty()) {
            int maxP = 1;
            bool small = true;
            for (int k : idx) {
                small = small && cfgs[k].nUE < (1 << 20) - 1;
                maxP = std::max(maxP, cfgs[k].nPreamble);
            }
            const size_t resident = (size_t)resident_workgroups(e, noma_kernel_blocks_per_cu(maxP));
            e->last.resident_limit = (int32_t)resident;
            // (measured at nUE = 100 000: 23.2 ms with 16 workgroups, 24.3 with 32, 26.6 with 8: 6 x nPreamble bins per mailbox)
            // (NOMA.c's own experiment — 10 seeds x the sweep = 100 trials in one call — measured 106 ms with one workgroup per trial, 61 ms with two:
            //  the clusters may fill the CUs the occupancy query admits, not half of them)
            const int G = small ? cluster_size(e, cfgs, idx, resident, 16, false) : 1; // (!small: 20-bit granule fields)
            std::vector<int> again;
            int rc = run_with_retries(e, cx, idx, G, LaunchOpts{}, &again);
            if (rc != PRACH_OK) return rc;
            if (!again.empty() && (G > 1 || cx.noma_ambiguous > 0)) { // one workgroup per trial waits for nobody; the host-built table needs no error band
                note_fallback(e, cx, "noma_kernel with one workgroup per trial and the host-built activation table", again, G);
                LaunchOpts host;
                host.host_act = true;
                rc = run_with_retries(e, cx, again, 1, host);
                if (rc != PRACH_OK) return rc;
            }
        }
    }
    for (int mode = 0; mode < 2; mode++) {
        std::vector<int> idx;
        for (int k = 0; k < n; k++)
            if (cfgs[k].rng_mode == mode && cfgs[k].variant != PRACH_VARIANT_NOMA_C) idx.push_back(k);
        if (idx.empty()) continue;
        // longest trials first: workgroups are dispatched in index order as CUs free up, so the tail of a
        // many-trial launch is made of the short trials
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
            auto work = [&](int k) { return (uint64_t)cfgs[k].nUE * (uint64_t)(cfgs[k].max_steps > 0 ? cfgs[k].max_steps : prach_max_time(&cfgs[k])); };
            return work(a) > work(b);
        });
        // trials only trial_kernel runs (index-ordered, exact, one workgroup each): the dormant per-sector grant path, sizes beyond the
        // cluster kernels' 20-bit granule fields / group tables — they leave the others on the cluster kernels
        std::vector<int> rest, sect, solo;
        for (int k : idx) {
            const bool sector = (cfgs[k].flags & PRACH_FLAG_SECTOR_GRANTS) != 0;
            const bool only_trial_kernel = sector || cfgs[k].nUE >= (1 << 20) - 1 || (mode == PRACH_RNG_GLIBC && cfgs[k].nUE > CLUSTER_GLIBC_MAX_UE);
            (sector && !e->opt_legacy && batch_eligible(e, cfgs[k]) ? sect : only_trial_kernel ? solo : rest).push_back(k);
        }
        std::vector<int> trial, sect_left;
        // the per-sector grant path: the batch kernel keeps the six budgets (one launch for these trials, one workgroup each; a trial whose draw-stream
        // window runs out retries there with a larger one, what exceeds a capacity of its resolver goes on to trial_kernel like any other trial)
        if (!sect.empty()) { int rc = descend_ladder(e, cx, sect, 1, sect_left); if (rc != PRACH_OK) return rc; }
        if (!e->opt_legacy && !rest.empty()) {
            // production path: cluster kernel, G workgroups per trial.  The workgroups of a cluster wait for each other, so
            // every cluster of the launch must be resident: G x trials <= what the occupancy query admits for this kernel
            // and LDS size (members of a cluster are consecutive workgroups: in-order dispatch completes whole clusters)
            int maxP = 1;
            for (int k : rest) maxP = std::max(maxP, cfgs[k].nPreamble);
            // (every cluster layout of this library takes more than half a CU's LDS: one workgroup per CU.  Asked of the runtime for the
            //  general kernel's smallest layout; the lean kernel and the LDS-resident layouts only ever need more LDS, never admit more)
            const size_t resident = (size_t)resident_workgroups(e, std::min(cluster_kernel_blocks_per_cu(maxP, mode, CLUSTER_REC_G16, 0), 1));
            e->last.resident_limit = (int32_t)resident;
            // (the clusters of a call may fill the CUs: 8 trials of 100 000 UEs run 52 ms on 8 x 32 workgroups — the lean kernel, one XCD each —
            //  against 78 ms on 8 x 16, 16 trials 78 ms on 16 x 16 against 96 ms on 16 x 8: scripts/gpu_probe_cluster_sizes.py)
            int rc = descend_ladder(e, cx, rest, cluster_size(e, cfgs, rest, resident, 32, true), trial);
            if (rc != PRACH_OK) return rc;
        } else trial = rest; // (engine option `legacy`: every trial on trial_kernel)
        trial.insert(trial.end(), solo.begin(), solo.end());
        trial.insert(trial.end(), sect_left.begin(), sect_left.end());
        int rc = run_with_retries(e, cx, trial, 0, LaunchOpts{}); // (trial_kernel has no capacity to exceed and no peer to wait for)
        if (rc != PRACH_OK) return rc;
    }
    uint64_t upd = 0;
    int worst = PRACH_OK;
    double seen = 0;
    for (int k = 0; k < n; k++) {
        upd += (uint64_t)cfgs[k].nUE * results[k].steps;
        if (results[k].status != PRACH_OK) worst = results[k].status;
        else if (cfgs[k].rng_mode == PRACH_RNG_GLIBC && cfgs[k].variant != PRACH_VARIANT_NOMA_C) seen = std::max(seen, (double)results[k].draws / (double)cfgs[k].nUE);
    }
    if (seen > 0) e->draws_per_ue_seen = seen; // (sizes the stream windows of the next call: stream_budget)
    e->last.kernel_ms = cx.kernel_ms;
    e->last.noma_host_ues = cx.noma_flagged;
    e->last.noma_gain_host_ues = cx.gain_host_ues;
    e->last.upload_ms = cx.upload_ms;
    e->last.updates = upd;
    if (red) {
        int rc = reduction_end(e, cx);
        e->last.*kind_of(*red).ms = cx.red_ms;
        if (rc != PRACH_OK) return rc;
    }
    e->last.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return worst;
}

// the groups of a reduction call: without a table trial k is group k, so there are n of them; with one, every entry names a group
static bool groups_ok(const int32_t *group, int ngroups, int n) {
    if (!group) return ngroups == n;
    for (int k = 0; k < n; k++) if (group[k] < 0 || group[k] >= ngroups) return false;
    return true;
}

// C++ exceptions (std::bad_alloc from the staging vectors) never cross the C boundary
#define PRACH_GUARD(body)                                                                              \
    try { body } catch (const std::bad_alloc &) {                                                       \
        std::fprintf(stderr, "[prach] out of host memory\n");                                          \
        return PRACH_ERR_DEVICE;                                                                       \
    } catch (...) { return PRACH_ERR_INTERNAL; }

extern "C" {

int prach_engine_create(int device, prach_engine **out) {
    if (!out) return PRACH_ERR_ARG;
    *out = nullptr;
    PRACH_GUARD(return engine_create_impl(device, out);)
}

void prach_engine_destroy(prach_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    free_arena(e);
    if (e->pinned) (void)hipHostFree(e->pinned);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->red_ev0) (void)hipEventDestroy(e->red_ev0);
    if (e->red_ev1) (void)hipEventDestroy(e->red_ev1);
    if (e->red_buf) (void)hipFree(e->red_buf);
    if (e->bulk_buf) (void)hipFree(e->bulk_buf);
    if (e->red_jobs_d) (void)hipFree(e->red_jobs_d);
    if (e->red_jobs_h) (void)hipHostFree(e->red_jobs_h);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int prach_engine_set(prach_engine *e, const char *key, int64_t value) {
    if (!e || !key) return PRACH_ERR_ARG;
    if (std::strcmp(key, "stream_factor") == 0) { e->opt_stream_factor = value; return PRACH_OK; }
    if (std::strcmp(key, "cluster") == 0) { if (value < 0 || value > CLUSTER_MAX_G) return PRACH_ERR_ARG; e->opt_cluster = value; return PRACH_OK; }
    if (std::strcmp(key, "legacy") == 0) { e->opt_legacy = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "dense") == 0) { e->opt_dense = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "wide_records") == 0) { e->opt_wide_records = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "pipeline") == 0) { e->opt_pipeline = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "resident") == 0) { if (value < 0) return PRACH_ERR_ARG; e->opt_resident = value; return PRACH_OK; }
    if (std::strcmp(key, "host_threads") == 0) { if (value < 0) return PRACH_ERR_ARG; e->opt_host_threads = value; return PRACH_OK; }
    if (std::strcmp(key, "lds_records") == 0) { e->opt_lds_records = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "fast") == 0) { e->opt_fast = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "vmm_fail_after") == 0) { if (value < 0) return PRACH_ERR_ARG; e->opt_vmm_fail_after = value; return PRACH_OK; }
    if (std::strcmp(key, "plain_arena") == 0) { if (e->arena_cap) return PRACH_ERR_ARG; e->opt_plain_arena = value != 0; return PRACH_OK; } // (before the first call only)
    if (std::strcmp(key, "noma_ambiguity_test") == 0) { e->opt_noma_ambiguity_test = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "noma_host_activation") == 0) { e->opt_noma_host_activation = value != 0; return PRACH_OK; }
    if (std::strcmp(key, "mem_budget_mb") == 0) { if (value <= 0) return PRACH_ERR_ARG; e->mem_budget = (size_t)value << 20; return PRACH_OK; } // (test hook: split launches)
    if (std::strcmp(key, "calendar_cap") == 0) { if (value < 0) return PRACH_ERR_ARG; e->opt_calendar_cap = value; return PRACH_OK; }
    if (std::strcmp(key, "batch_waves") == 0) { if (value != 0 && value != 8 && value != 16) return PRACH_ERR_ARG; e->opt_batch_waves = value; return PRACH_OK; }
    if (std::strcmp(key, "dist_scheme") == 0) { if (value < 0 || value > 2) return PRACH_ERR_ARG; e->opt_dist_scheme = value; return PRACH_OK; }
    if (std::strcmp(key, "timeline_scheme") == 0) { if (value < 0 || value > 1) return PRACH_ERR_ARG; e->opt_timeline_scheme = value; return PRACH_OK; }
    if (std::strcmp(key, "noma_timeline_window") == 0) { if (value < 0 || value > NTL_WINDOW_MAX) return PRACH_ERR_ARG; e->opt_noma_timeline_window = value ? value : NTL_WINDOW; return PRACH_OK; }
    if (std::strcmp(key, "summary_threads") == 0) { if (value != 0 && value != 512 && value != 1024) return PRACH_ERR_ARG; e->opt_summary_threads = value ? value : 1024; return PRACH_OK; }
    if (std::strcmp(key, "pick_threads") == 0) { if (value != 0 && value != 512 && value != 1024) return PRACH_ERR_ARG; e->opt_pick_threads = value ? value : 1024; return PRACH_OK; }
    if (std::strcmp(key, "trace_scheme") == 0) { if (value < 0 || value > 1) return PRACH_ERR_ARG; e->opt_trace_scheme = value; return PRACH_OK; }
    if (std::strcmp(key, "xtab_scheme") == 0) { if (value < 0 || value > 1) return PRACH_ERR_ARG; e->opt_xtab_scheme = value; return PRACH_OK; }
    if (std::strcmp(key, "sojourn_scheme") == 0) { if (value < 0 || value > 1) return PRACH_ERR_ARG; e->opt_sojourn_scheme = value; return PRACH_OK; }
    if (std::strcmp(key, "xcd_pack") == 0) { e->opt_xcd_pack = value != 0; return PRACH_OK; }
    return PRACH_ERR_ARG;
}

int prach_device_glibc_stream(prach_engine *e, uint32_t seed, uint64_t first, uint64_t n, int32_t *out) {
    if (!e || !out || n == 0) return PRACH_ERR_ARG;
    PRACH_GUARD(
        HIPCHK(hipSetDevice(e->device));
        const size_t nchunks = (n + STREAM_CHUNK - 1) / STREAM_CHUNK;
        const size_t need = align_up(4 * 31 * nchunks, 256) + 4 * (n + 2);
        { int rc = ensure_arena(e, need); if (rc != PRACH_OK) return rc; }
        std::vector<uint32_t> seeds(31 * nchunks);
        prach_internal_glibc_seeds(seed, first, nchunks, STREAM_CHUNK, seeds.data());
        HIPCHK(hipMemcpy(e->arena, seeds.data(), 4 * 31 * nchunks, hipMemcpyHostToDevice));
        int *dout = reinterpret_cast<int *>(e->arena + align_up(4 * 31 * nchunks, 256));
        HIPCHK(launch_glibc_stream(reinterpret_cast<const unsigned *>(e->arena), dout, n, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(out, dout, 4 * n, hipMemcpyDeviceToHost));
        return PRACH_OK;
    )
}

static int activation_table_device_impl(prach_engine *e, const prach_cfg *cfg, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                   uint32_t *ndraws, uint8_t *flagged) {
    if (!e || !cfg || !preamble0 || !sector || !gain || !lgain || !ndraws) return PRACH_ERR_ARG;
    { int v = prach_cfg_validate(cfg); if (v != PRACH_OK) return v; }
    if (cfg->variant != PRACH_VARIANT_NOMA_C || cfg->rng_mode != PRACH_RNG_PHILOX) return PRACH_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    const size_t n = (size_t)cfg->nUE;
    size_t o = align_up(sizeof(TrialDev), 256);
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    const size_t oflags = take(4 * (2 + 2 * (size_t)NOMA_ACT_FLAG_CAP)), opre = take(4 * n), osec = take(4 * n), ogain = take(8 * n), olg = take(8 * n), ond = take(4 * n);
    { int rc = ensure_arena(e, o); if (rc != PRACH_OK) return rc; }
    char *const A = e->arena;
    TrialDev d;
    std::memset(&d, 0, sizeof(d));
    d.variant = cfg->variant; d.nUE = cfg->nUE; d.nP = cfg->nPreamble; d.seed_lo = (unsigned)cfg->seed; d.seed_hi = (unsigned)(cfg->seed >> 32);
    d.cell_radius = cfg->cellRadius;
    d.n_pre0 = reinterpret_cast<const int *>(A + opre); d.n_sector = reinterpret_cast<const int *>(A + osec);
    d.n_gain = reinterpret_cast<const double *>(A + ogain); d.n_lgain = reinterpret_cast<const double *>(A + olg);
    d.n_nd0 = reinterpret_cast<const unsigned *>(A + ond);
    HIPCHK(hipMemcpyAsync(A, &d, sizeof(d), hipMemcpyHostToDevice, e->stream)); // (on the engine's stream, like the kernel behind them)
    HIPCHK(hipMemsetAsync(A + oflags, 0, 8, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int idx0 = 0;
    std::vector<ActTab> tabs(1, ActTab{A + opre, A + osec, A + ogain, A + olg, A + ond});
    std::vector<std::pair<int, int>> fl;
    int nflagged = 0;
    { int rc = noma_device_activation(e, reinterpret_cast<const TrialDev *>(A), cfg, &idx0, 1, tabs, reinterpret_cast<unsigned *>(A + oflags), &fl, nflagged); if (rc != PRACH_OK) return rc == NOMA_ACT_OVERFLOW_RC ? PRACH_ERR_INTERNAL : rc; }
    HIPCHK(hipMemcpy(preamble0, A + opre, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sector, A + osec, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(gain, A + ogain, 8 * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lgain, A + olg, 8 * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ndraws, A + ond, 4 * n, hipMemcpyDeviceToHost));
    if (flagged) {
        std::memset(flagged, 0, n);
        for (const auto &f : fl) flagged[f.second] = 1;
    }
    return PRACH_OK;
}

int prach_noma_activation_table_device(prach_engine *e, const prach_cfg *cfg, int32_t *preamble0, int32_t *sector, double *gain, double *lgain,
                                       uint32_t *ndraws, uint8_t *flagged) {
    PRACH_GUARD(return activation_table_device_impl(e, cfg, preamble0, sector, gain, lgain, ndraws, flagged);)
}

int prach_last_timing(const prach_engine *e, prach_timing *out) {
    if (!e || !out) return PRACH_ERR_ARG;
    *out = e->last;
    return PRACH_OK;
}

int prach_run_trials(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs) {
    if (!e || !cfgs || !results || n <= 0) return PRACH_ERR_ARG;
    PRACH_GUARD(return run_trials_impl(e, cfgs, n, results, ue_logs);)
}

// a trial the NOMA menu's device calls take: NOMA.c with Philox (the reference-stream launches, run_noma_glibc, lay out no job the menu's kernels read: not wired to the menu)
static bool noma_device_cfg(const prach_cfg &c) { return c.variant == PRACH_VARIANT_NOMA_C && c.rng_mode != PRACH_RNG_GLIBC; }

// The grouped kinds (csrc/prach_grouped.h): the Red of each, in the order of PRACH_G_*.  What else the host side knows about a kind — the sizes, the shape of its
// arrays, where ngroups and the reserved words sit in its spec, the trials it takes — is its row of GROUPED in prach_host.c
static const Red GROUPED_RED[PRACH_G_KINDS] = {Red::dist, Red::timeline, Red::sojourn, Red::trace, Red::xtab, Red::noma_census, Red::noma_trace, Red::noma_timeline};
static const Red GROUPED_RED_MORE[PRACH_G_MORE_END - PRACH_G_MORE] = {Red::noma_gain}; // ... and of the enumerators from PRACH_G_MORE on
static Red grouped_red(int kind) { return kind < PRACH_G_KINDS ? GROUPED_RED[kind] : GROUPED_RED_MORE[kind - PRACH_G_MORE]; } // (a kind that has a row)

// THE refusal sequence of every grouped call.  Arguments first (pointers, spec, ngroups, reserved, group ids), then what is not supported (the trials' programs,
// then the cap of 2^27 words = 1 GiB of device buffer), then the missing engine: spec, groups and variants are judged first, what they ask for does not depend
// on a device
int prach_internal_grouped_run(int kind, prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const void *spec,
                               const int32_t *group, void *groups, uint64_t *const arrays[]) {
    const prach_grouped_row *const k = prach_internal_grouped_row(kind);
    size_t words[PRACH_G_MAX_ARRAYS];
    const int narrays = k ? k->shape(spec, words) : 0;
    if (!cfgs || !results || n <= 0 || !narrays || !groups || !arrays) return PRACH_ERR_ARG;
    uint64_t group_words = 0;
    for (int q = 0; q < narrays; q++) {
        if (!arrays[q]) return PRACH_ERR_ARG;
        group_words += words[q];
    }
    const int ngroups = *reinterpret_cast<const int32_t *>(static_cast<const char *>(spec) + k->ngroups_at);
    const int32_t *const reserved = reinterpret_cast<const int32_t *>(static_cast<const char *>(spec) + k->reserved_at);
    if (ngroups < 1) return PRACH_ERR_ARG;
    for (int r = 0; r < k->reserved_words; r++) if (reserved[r] != 0) return PRACH_ERR_ARG;
    if (!groups_ok(group, ngroups, n)) return PRACH_ERR_ARG;
    for (int t = 0; t < n; t++) // (NOMA.c has a menu and a resolver of its own, and its kinds take no other program: include/prach.h)
        if (k->trials == PRACH_G_TRIALS_NOT_NOMA_C ? cfgs[t].variant == PRACH_VARIANT_NOMA_C : k->trials == PRACH_G_TRIALS_NOMA_C_PHILOX && !noma_device_cfg(cfgs[t]))
            return PRACH_ERR_UNSUPPORTED;
    if ((uint64_t)ngroups * group_words > (1ull << 27)) return PRACH_ERR_UNSUPPORTED;
    if (!e) return PRACH_ERR_ARG;
    Reduction red{.kind = grouped_red(kind), .group = group, .ngroups = ngroups, .out = {}, .spec = spec, .groups = groups};
    for (int q = 0; q < narrays; q++) red.out[q] = arrays[q];
    PRACH_GUARD(return run_trials_impl(e, cfgs, n, results, ue_logs, &red);)
}

int prach_run_trials_dist(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_dist_spec *spec,
                          const int32_t *group, prach_dist *dist, uint64_t *delay_hist, uint64_t *ptc_hist) {
    uint64_t *const arrays[] = {delay_hist, ptc_hist};
    return prach_internal_grouped_run(PRACH_G_DIST, e, cfgs, n, results, ue_logs, spec, group, dist, arrays);
}
int prach_run_trials_timeline(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_timeline_spec *spec,
                              const int32_t *group, prach_timeline *tl, uint64_t *arrivals, uint64_t *success, uint64_t *sojourn_sum, uint64_t *timer_sum, uint64_t *done) {
    uint64_t *const arrays[] = {arrivals, success, sojourn_sum, timer_sum, done};
    return prach_internal_grouped_run(PRACH_G_TIMELINE, e, cfgs, n, results, ue_logs, spec, group, tl, arrays);
}
int prach_run_trials_sojourn(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_sojourn_spec *spec,
                             const int32_t *group, prach_sojourn *sj, uint64_t *hist, uint64_t *row_arrived, uint64_t *row_delay_overflow) {
    uint64_t *const arrays[] = {hist, row_arrived, row_delay_overflow};
    return prach_internal_grouped_run(PRACH_G_SOJOURN, e, cfgs, n, results, ue_logs, spec, group, sj, arrays);
}
int prach_run_trials_trace(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_trace_spec *spec,
                           const int32_t *group, prach_trace *tr, uint64_t *calls, uint64_t *singles, uint64_t *txop, uint64_t *collisions) {
    uint64_t *const arrays[] = {calls, singles, txop, collisions};
    return prach_internal_grouped_run(PRACH_G_TRACE, e, cfgs, n, results, ue_logs, spec, group, tr, arrays);
}
int prach_run_trials_xtab(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_xtab_spec *spec,
                          const int32_t *group, prach_xtab *xt, uint64_t *cells) {
    return prach_internal_grouped_run(PRACH_G_XTAB, e, cfgs, n, results, ue_logs, spec, group, xt, &cells);
}
int prach_run_trials_noma_census(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_xtab_spec *spec,
                                 const int32_t *group, prach_noma_census *cs, uint64_t *cells) {
    return prach_internal_grouped_run(PRACH_G_NOMA_CENSUS, e, cfgs, n, results, ue_logs, spec, group, cs, &cells);
}
int prach_run_trials_noma_trace(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_noma_trace_spec *spec,
                                const int32_t *group, prach_noma_trace *tr, uint64_t *const series[6]) {
    return prach_internal_grouped_run(PRACH_G_NOMA_TRACE, e, cfgs, n, results, ue_logs, spec, group, tr, series);
}
int prach_run_trials_noma_timeline(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_noma_timeline_spec *spec,
                                   const int32_t *group, prach_noma_timeline *tl, uint64_t *const series[6]) {
    return prach_internal_grouped_run(PRACH_G_NOMA_TIMELINE, e, cfgs, n, results, ue_logs, spec, group, tl, series);
}

int prach_run_trials_noma_gain(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_noma_gain_spec *spec,
                               const int32_t *group, prach_noma_gain *g, uint64_t *const series[6]) {
    return prach_internal_grouped_run(PRACH_G_NOMA_GAIN, e, cfgs, n, results, ue_logs, spec, group, g, series);
}

int prach_dist_tile_ues(void) { return DIST_TILE; }

int prach_timeline_tile_ues(void) { return TL_TILE; }
int prach_timeline_window_bins(void) { return TL_WINDOW; }

int prach_run_trials_summary(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_summary_spec *spec,
                             prach_trial_summary *rows) {
    // (spec and variants are judged first: what they ask for does not depend on a device)
    if (!cfgs || !results || n <= 0 || !spec || !rows) return PRACH_ERR_ARG;
    if (spec->nq < 1 || spec->nq > PRACH_SUMMARY_MAX_Q || spec->reserved[0] || spec->reserved[1] || spec->reserved[2]) return PRACH_ERR_ARG;
    for (int l = 0; l < spec->nq; l++) if (spec->permille[l] < 1 || spec->permille[l] > 1000) return PRACH_ERR_ARG;
    for (int k = 0; k < n; k++) if (cfgs[k].variant == PRACH_VARIANT_NOMA_C) return PRACH_ERR_UNSUPPORTED; // (NOMA.c has a menu of its own: include/prach.h)
    if (!e) return PRACH_ERR_ARG;
    static_assert(SM_MAX_VALUE == 65535, "prach_summary_max_value (prach_host.c) states the kernel's bound");
    const Reduction red{.kind = Red::summary, .group = nullptr, .ngroups = n, .out = {}, .spec = spec, .groups = rows};
    PRACH_GUARD(return run_trials_impl(e, cfgs, n, results, ue_logs, &red);)
}

int prach_trace_tile_subframes(void) { return TR_TILE; }

int prach_sojourn_tile_ues(void) { return TL_TILE; }
int prach_sojourn_window_words(void) { return SJ_WINDOW_WORDS; }

int prach_run_trials_pick(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_pick_spec *spec,
                          prach_pick *picks, prach_pick_row *rows) {
    // (spec and variants are judged first: what they ask for does not depend on a device)
    if (!cfgs || !results || n <= 0 || !spec || !picks || !rows || !prach_internal_pick_spec_ok(spec)) return PRACH_ERR_ARG;
    for (int k = 0; k < n; k++) if (cfgs[k].variant == PRACH_VARIANT_NOMA_C) return PRACH_ERR_UNSUPPORTED; // (NOMA.c has a menu of its own: include/prach.h)
    if ((uint64_t)n * ((uint64_t)spec->k * PK_ROW_WORDS + PK_SCALARS) > (1ull << 27)) return PRACH_ERR_UNSUPPORTED;
    if (!e) return PRACH_ERR_ARG;
    const Reduction red{.kind = Red::pick, .group = nullptr, .ngroups = n, .out = {reinterpret_cast<uint64_t *>(rows)}, .spec = spec, .groups = picks};
    PRACH_GUARD(return run_trials_impl(e, cfgs, n, results, ue_logs, &red);)
}

// what the two columns entry points share: the refusals that need no device, then the table of first rows.  dev: the destination is the caller's device memory
// The headers of a columns call, typed: the header's type says which menu the call is over (is_noma: THE NOMA MENU, whose refusals are the census's)
struct ColumnsHdr {
    void *p;
    bool is_noma;
    ColumnsHdr(prach_columns *h) : p(h), is_noma(false) {}
    ColumnsHdr(prach_noma_columns *h) : p(h), is_noma(true) {}
};
static int run_trials_columns(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_columns_spec *spec,
                              ColumnsHdr h, void *out, uint64_t rows_cap, bool dev) {
    const bool noma = h.is_noma;
    void *const hdr = h.p;
    // (spec, sizes and variants are judged first: what they ask for does not depend on a device)
    if (!cfgs || !results || n <= 0 || !hdr || !out || !(noma ? prach_internal_noma_columns_spec_ok(spec) : prach_internal_columns_spec_ok(spec))) return PRACH_ERR_ARG;
    std::vector<uint64_t> offset((size_t)n);
    uint64_t rows = 0;
    for (int k = 0; k < n; k++) {
        if (cfgs[k].nUE < 0) return PRACH_ERR_ARG;
        offset[(size_t)k] = rows;
        rows += (uint64_t)cfgs[k].nUE;
    }
    if (rows_cap < rows) return PRACH_ERR_ARG;
    for (int k = 0; k < n; k++) if (noma ? !noma_device_cfg(cfgs[k]) : cfgs[k].variant == PRACH_VARIANT_NOMA_C) return PRACH_ERR_UNSUPPORTED; // (the menu is the other programs': include/prach.h)
    if (rows_cap > PRACH_COL_MAX_WORDS || (uint64_t)spec->ncols * rows_cap > PRACH_COL_MAX_WORDS) return PRACH_ERR_UNSUPPORTED;
    if (!e) return PRACH_ERR_ARG;
    if (dev) { // device memory of the engine's device, all of it: asked before the fill and before any launch
        HIPCHK(hipSetDevice(e->device));
        hipPointerAttribute_t attr{};
        void *base = nullptr;
        size_t size = 0;
        const size_t span = 4 * ((size_t)(spec->ncols - 1) * (size_t)rows_cap + (size_t)rows);
        if (hipPointerGetAttributes(&attr, out) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != e->device ||
            hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t *>(&base), &size, out) != hipSuccess || (reinterpret_cast<uintptr_t>(out) & 3) != 0 ||
            static_cast<char *>(out) + span > static_cast<char *>(base) + size) {
            (void)hipGetLastError();
            return PRACH_ERR_ARG;
        }
    }
    Reduction red{.kind = noma ? Red::noma_columns : Red::columns, .group = nullptr, .ngroups = n, .out = {}, .spec = spec, .groups = hdr};
    (dev ? red.bulk_dev : red.bulk_host) = out;
    red.bulk_width = 4 * (size_t)rows; red.bulk_rows = rows ? (size_t)spec->ncols : 0; red.bulk_pitch = 4 * (size_t)rows_cap; red.bulk_fill = 0xff; // -1
    if (!rows) red.bulk_width = 0;
    red.table = offset.data(); red.table_bytes = 8 * offset.size();
    return run_trials_impl(e, cfgs, n, results, ue_logs, &red);
}

int prach_run_trials_columns(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_columns_spec *spec,
                             prach_columns *hdr, int32_t *out, uint64_t rows_cap) {
    PRACH_GUARD(return run_trials_columns(e, cfgs, n, results, ue_logs, spec, hdr, out, rows_cap, false);)
}

int prach_run_trials_columns_device(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_columns_spec *spec,
                                    prach_columns *hdr, void *dev_out, uint64_t rows_cap) {
    PRACH_GUARD(return run_trials_columns(e, cfgs, n, results, ue_logs, spec, hdr, dev_out, rows_cap, true);)
}

int prach_run_trials_noma_columns(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_columns_spec *spec,
                                  prach_noma_columns *hdr, int32_t *out, uint64_t rows_cap) {
    PRACH_GUARD(return run_trials_columns(e, cfgs, n, results, ue_logs, spec, hdr, out, rows_cap, false);)
}

int prach_run_trials_noma_columns_device(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs,
                                         const prach_columns_spec *spec, prach_noma_columns *hdr, void *dev_out, uint64_t rows_cap) {
    PRACH_GUARD(return run_trials_columns(e, cfgs, n, results, ue_logs, spec, hdr, dev_out, rows_cap, true);)
}

int prach_run_trials_noma_summary(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_noma_summary_spec *spec,
                                  prach_noma_trial_summary *rows) {
    // (spec and variants are judged first: what they ask for does not depend on a device)
    if (!cfgs || !results || n <= 0 || !spec || !rows || !prach_internal_noma_summary_spec_ok(spec)) return PRACH_ERR_ARG;
    for (int k = 0; k < n; k++) if (!noma_device_cfg(cfgs[k])) return PRACH_ERR_UNSUPPORTED;
    if (!e) return PRACH_ERR_ARG;
    const Reduction red{.kind = Red::noma_summary, .group = nullptr, .ngroups = n, .out = {}, .spec = spec, .groups = rows};
    PRACH_GUARD(return run_trials_impl(e, cfgs, n, results, ue_logs, &red);)
}

int prach_run_trials_noma_pick(prach_engine *e, const prach_cfg *cfgs, int n, prach_result *results, prach_ue_log *const *ue_logs, const prach_pick_spec *spec,
                               prach_pick *picks, prach_pick_row *rows) {
    // (spec and variants are judged first: what they ask for does not depend on a device)
    if (!cfgs || !results || n <= 0 || !spec || !picks || !rows || !prach_internal_noma_pick_spec_ok(spec)) return PRACH_ERR_ARG;
    for (int k = 0; k < n; k++) if (!noma_device_cfg(cfgs[k])) return PRACH_ERR_UNSUPPORTED;
    if ((uint64_t)n * ((uint64_t)spec->k * PK_ROW_WORDS + PK_SCALARS) > (1ull << 27)) return PRACH_ERR_UNSUPPORTED;
    if (!e) return PRACH_ERR_ARG;
    const Reduction red{.kind = Red::noma_pick, .group = nullptr, .ngroups = n, .out = {reinterpret_cast<uint64_t *>(rows)}, .spec = spec, .groups = picks};
    PRACH_GUARD(return run_trials_impl(e, cfgs, n, results, ue_logs, &red);)
}

int prach_noma_timeline_tile_ues(void) { return TL_TILE; }
int prach_noma_timeline_window_bins(void) { return NTL_WINDOW; }
int prach_noma_gain_tile_ues(void) { return TL_TILE; }
int prach_noma_gain_lds_max_bins(void) { return NG_LDS_MAX_BINS; }
int prach_noma_trace_tile_rows(void) { return NT_TILE; }
int prach_noma_census_tile_ues(void) { return TL_TILE; }
int prach_columns_tile_ues(void) { return TL_TILE; }
int prach_xtab_tile_ues(void) { return TL_TILE; }
int prach_xtab_window_words(void) { return XT_WINDOW_WORDS; }

} // extern "C"
