// prach_exchange.h — the exchange protocol of a cluster of workgroups, ONE copy (device only): the granule, its loads and stores, the bounded
// wait, the XCD-packed block mapping and the same-XCD handshake.  Included by prach_cluster.hip, prach_lcluster.hip and prach_noma.hip.
#pragma once
#include "prach_device_fn.h"

namespace prach {

// Exchange granule: ONE naturally aligned 8-byte write-through store {20-bit value | tag[11:0]} {20-bit value | tag[15:12]}.
// Every granule carries the subframe tag (t+1 <= 60001 fits 16 bits), so it validates itself: the consumer
// re-reads until the tag matches — no drain, no flag, no fence (cdna_hip_programming.md G16, R2).
constexpr unsigned GR_NONE = 0xFFFFFu;      // "no UE index" in a 20-bit value
constexpr unsigned SPIN_LIMIT = 1u << 22;   // re-reads of one granule before the wait gives up
__device__ __forceinline__ long long mk_granule(unsigned lo20, unsigned hi20, unsigned tag) {
    const unsigned w0 = (lo20 & 0xFFFFFu) | ((tag & 0xFFFu) << 20), w1 = (hi20 & 0xFFFFFu) | (((tag >> 12) & 0xFu) << 20);
    return (long long)(((unsigned long long)w1 << 32) | w0);
}
__device__ __forceinline__ bool granule_ok(long long g, unsigned tag) {
    const unsigned w0 = (unsigned)g, w1 = (unsigned)((unsigned long long)g >> 32);
    return (w0 >> 20) == (tag & 0xFFFu) && ((w1 >> 20) & 0xFu) == ((tag >> 12) & 0xFu);
}
// shared words: every access is a device-scope relaxed atomic == global_load/store ... sc1
__device__ __forceinline__ long long ld_sc1_64(const PRACH_G long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1_64(PRACH_G long long *p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// A cluster whose workgroups have VERIFIED (same_xcd_handshake, before the step loop) that they all run on one XCD shares that XCD's L2: its
// granule stores may then stay in L2 (workgroup-scope store: no write-through to the fabric), where the peers' `sc1` loads — which
// bypass only the per-CU L1 — find them after an L2 round trip instead of a fabric one (guide: `sc1` stores DROP the line from the
// XCD's L2, plain / `sc0` stores KEEP it).  Any other placement keeps the write-through stores.
__device__ __forceinline__ void st_gr(const bool same_xcd, PRACH_G long long *p, long long v) {
    if (same_xcd) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// bounded re-read of one granule until it carries `tag`
__device__ __forceinline__ long long wait_granule(const PRACH_G long long *p, unsigned tag, int *status_word) {
    long long g = ld_sc1_64(p);
    unsigned spins = 0;
    while (!granule_ok(g, tag)) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > SPIN_LIMIT) { *status_word = PRACH_ERR_TIMEOUT; break; } // peer not resident? the engine reruns the trial
        g = ld_sc1_64(p);
    }
    return g;
}

// Block -> (trial T, workgroup b of its cluster); false for a block past the last trial.  Plain: a cluster = G CONSECUTIVE blocks (in-order
// dispatch completes whole clusters).  XCD-packed: blocks bx and bx + 8 are dealt to the same XCD (observed round-robin dispatch, for speed
// only — the handshake below checks it), so a cluster is made of the blocks of equal bx % 8 of one chunk of 8 G blocks, and eight clusters —
// one per XCD — share a chunk.
__device__ __forceinline__ bool cluster_block(const int G, const int xpack, const int ntrials, int &T, int &b) {
    T = blockIdx.x / G; b = blockIdx.x % G;
    if (xpack) {
        const int chunk = blockIdx.x / (8 * G), within = blockIdx.x % (8 * G);
        T = chunk * 8 + (within & 7); b = within >> 3;
        if (T >= ntrials) return false;
    }
    return true;
}

// Same-XCD handshake (whole workgroup, G <= 64): every workgroup publishes the id of the XCD it runs on (write-through granule, tag 0xFFFF, in the
// header of its parity-1 mailbox — first used by subframe 1, which no workgroup reaches before every peer is past this point, because
// subframe 0's exchange needs every peer's subframe-0 granules) and reads all G of them: the cluster keeps its granules in L2 only if they
// are all equal.  Every workgroup reads the same G values, so all decide alike.  hs: header of workgroup 0's parity-1 mailbox; stride:
// granules per mailbox (its type is the caller's address arithmetic); verdict: one LDS word.
template <class S>
__device__ __forceinline__ bool same_xcd_handshake(PRACH_G long long *const hs, const S stride, const int b, const int G, int *const status_word, int *const verdict) {
    const int tid = threadIdx.x;
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xfu;
    if (tid == 0) st_sc1_64(hs + (S)b * stride, mk_granule(xcc, 0u, 0xFFFFu));
    if (tid < 64) {
        bool same = true;
        if (tid < G) same = ((unsigned)wait_granule(hs + (S)tid * stride, 0xFFFFu, status_word) & 0xFFFFFu) == xcc;
        const bool all = __ballot(!same) == 0ull;
        if (tid == 0) *verdict = all ? 1 : 0;
    }
    __syncthreads();
    return *verdict != 0 && *status_word == PRACH_OK;
}

} // namespace prach
