"""The cases of the exchange roles of prach::lcluster_kernel (prach_lcluster.hip: bucket roles packed a byte each, event roles derived from the thread
index, the second event role behind one wave-uniform test).  A repacked role can only go wrong where it is live:

  G x nPreamble > 1024     a thread's second bucket role          G > 32     the second event role (workgroups 32 .. G - 1)
  G x nPreamble > 2048     its third                              G <= 32    that role skipped (the headline's shape)
  G x nPreamble > 3072     the tail loop behind the three roles

A case is (cluster size G, nUE, overrides); its trials are both variants in both RNG modes (lcluster_kernel<false> and <true>), each uncut and stopped at
CUTS.  nUE lies between 64 G and 3 x 64 G, so every workgroup owns at least one 64-UE group, and nGrantUL is 3 to 6, so that a loaded trial has callers,
UEs that leave their bucket, reset candidates and grants all the time.  Plain data and the oracle's census: no GPU, no package import.
tests/test_lcluster_roles_cases_cpu.py asserts what the trials contain; tests/tools/gpu_lcluster_roles.py runs them on the GPU."""
import numpy as np
import ctypes as C

from oracle import binding as ob
import trace_ref

SEED = 900
CASES = [
    ("g24_p54", 24, 3000, dict(nPreamble=54, nGrantUL=4)),   # 1 296 bucket granules: second bucket role
    ("g40_p54", 40, 5000, dict(nPreamble=54, nGrantUL=5)),   # 2 160: third bucket role; workgroups 32 .. 39 on the second event role
    ("g64_p54", 64, 8000, dict(nPreamble=54, nGrantUL=6)),   # 3 456: the tail loop; every thread on the second event role
    ("g64_p8", 64, 6000, dict(nPreamble=8, nGrantUL=3)),     # 512: one bucket role only
    ("g64_p64", 64, 8000, dict(nPreamble=64, nGrantUL=6)),   # 4 096: every row of the bucket tables
    ("g32_p54", 32, 4000, dict(nPreamble=54, nGrantUL=4)),   # the headline's shape: no second event role
]
CASE = {name: (G, n, kw) for name, G, n, kw in CASES}
CUTS = (6, 62, 333, 1204, 2500)  # last subframes 5, 61, 332, 1203, 2499: every residue of 5


def live(name):
    """Which roles the case's shape makes live: dict(bucket_roles 1..3, tail, ev1)."""
    G, _, kw = CASE[name]
    n = G * kw["nPreamble"]
    return dict(bucket_roles=min(3, (n + 1023) // 1024), tail=n > 3072, ev1=G > 32)


def trials(name):
    """[(cut or None, trial)] of a case: trials are gpu_kernel_matrix's tuples (program, variant, nUE, overrides, rng, seed)."""
    G, n, kw = CASE[name]
    out = []
    for v in (0, 1):
        for rng in (0, 1):
            base = ("beta", v, n, dict(kw), rng, SEED + v)
            out.append((None, base))
            out += [(c, (base[0], v, n, dict(kw, max_steps=c), rng, SEED + v)) for c in CUTS]
    return out


def census(name, variant, rng):
    """dict(calls, singles, redraws per subframe; steps, aT) of the uncut oracle run of one trial of the case."""
    G, n, kw = CASE[name]
    L = ob.lib()
    L.oracle_set_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.oracle_set_census.restype = None
    T = 10000
    redraws, calls, singles = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32)
    L.oracle_set_census(redraws.ctypes.data, singles.ctypes.data, calls.ctypes.data, T)
    try:
        res = trace_ref.run((variant, n, kw, rng, SEED + variant))
    finally:
        L.oracle_set_census(None, None, None, 0)
    steps = int(res.steps)
    return dict(calls=calls[:steps].astype(np.int64), singles=singles[:steps].astype(np.int64), redraws=redraws[:steps].astype(np.int64), steps=steps,
                aT=kw.get("accessTime", 5), nSuccessUE=int(res.nSuccessUE))


def counts(c):
    """Subframes with calls, with singleton calls, and with leavers: a preamble drawn off the arrival subframe (t % accessTime != 0) is drawn by a UE
    that gives up the bucket it was matched in (RAR window over, Msg3 timed out) — arrivals draw their first one at t % accessTime == 0."""
    off = (np.arange(c["steps"]) % c["aT"]) != 0
    return dict(calls=int((c["calls"] > 0).sum()), singles=int((c["singles"] > 0).sum()), leavers=int(((c["redraws"] > 0) & off).sum()))
