"""The small __device__ building blocks every trial kernel is made of (prach_device_fn.h, prach_exchange.h, the record helpers of prach_cluster.hip), away
from every trial: a deterministic generator of cases no Monte-Carlo trial produces, their references — plain Python / numpy, the pinned oracle's Philox —
and the glue around tests/tools/gpu_prims_harness.hip (case file, result file, one child process per section and build).  Shared by
tests/test_prims_cases_cpu.py and tests/test_gpu_prims_synthetic.py.  No GPU here; the constants of the product's headers come from
`gpu_prims_harness --constants`, and the harness's `--host` mode runs whatever is host-callable on the CPU (the branched per-UE body is the reference of
the mask section)."""
import ctypes
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import harness as H
from harness import constants as harness_constants  # noqa: F401

MAGIC = 0x50524D53
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HARNESS = "gpu_prims_harness.hip"
CSRC = os.path.join(ROOT, "5g-nr-randomaccess_amd", "csrc")
SECTIONS = dict(philox=1, masks=2, wave=3, mod=4, sector=5, granule=6, blocks=7, hot=8, pack=9)
PRODUCT_FLAGS = ["-ffp-contract=off"]  # on top of harness.FLAGS
NOBITOP3_FLAGS = ["-DPRACH_NO_BITOP3", "-Xclang", "-target-feature", "-Xclang", "-bitop3-insts"]  # csrc/Makefile, NOBITOP3=1
BUILDS = ("product", "nobitop3")
U32 = 0xFFFFFFFF
INT_MIN, INT_MAX = -2**31, 2**31 - 1


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    """Compiles tests/tools/gpu_prims_harness.hip twice, side by side: with the product's flags and with the NOBITOP3 flags of csrc/Makefile on top.
    {build name: executable}."""
    with ThreadPoolExecutor(len(BUILDS)) as pool:
        exes = pool.map(lambda b: H.build(HARNESS, out_dir, PRODUCT_FLAGS + (NOBITOP3_FLAGS if b == "nobitop3" else []), f"gpu_prims_harness_{b}"), BUILDS)
        return dict(zip(BUILDS, exes))


def write_case(path, section, n, payload, p3=0, p4=0):
    h = np.zeros(16, dtype="<i4")
    h[:5] = [MAGIC, SECTIONS[section], n, p3, p4]
    with open(path, "wb") as f:
        f.write(h.tobytes())
        for a in payload:  # (values given as int32 or as uint32: the same 32 bits)
            f.write((np.ascontiguousarray(a).astype(np.int64) & U32).astype("<u4").tobytes())


def read_result(path, section, host, n):
    r = np.fromfile(path, dtype="<u4")
    assert r[:4].tolist() == [MAGIC, SECTIONS[section], host, n], r[:4].tolist()
    return r[4:]


def run_harness(exe, section, case_path, result_path, host=False, timeout=120):
    """One section in a fresh child process (harness.run)."""
    H.run(exe, (["--host"] if host else []) + [SECTIONS[section], case_path, result_path], timeout)


def u32(a):
    return np.asarray(a, dtype=np.int64) & U32


def as_i32(a):
    """0 .. 2^32 - 1 -> the int32 with the same bits."""
    a = np.asarray(a, dtype=np.int64) & U32
    return np.where(a >= 2**31, a - 2**32, a).astype(np.int64)


# ---- 1 philox ---------------------------------------------------------------------------------------------------------------------------------------------
PHILOX_KAT = [  # Random123 kat_vectors, philox4x32-10: counter, key, expected (as tests/test_oracle_rng.py pins them on the oracle)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
PHILOX_WALK = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)
PHILOX_N_RANDOM = 14000


def philox_cases():
    """rows of (k0, k1, c0, c1, c2, c3) = (seed_lo, seed_hi, ue, k, nUE, variant), uint32; at most 20 000."""
    rng = np.random.default_rng(31)
    rows = [key + ctr for ctr, key, _ in PHILOX_KAT]
    fixed = tuple(int(v) for v in rng.integers(0, 2**32, 6))
    for bg in ((0,) * 6, fixed):
        for word in range(6):
            for v in PHILOX_WALK:
                r = list(bg)
                r[word] = v
                rows.append(tuple(r))
    for c1 in (0xFFFFFFFE, 0xFFFFFFFF):  # the second draw of _x2 is at (c1 + 1) mod 2^32
        rows.append((0, 0, 0, c1, 0, 0))
        for _ in range(40):
            r = [int(v) for v in rng.integers(0, 2**32, 6)]
            r[3] = c1
            rows.append(tuple(r))
    rows += [tuple(int(v) for v in r) for r in rng.integers(0, 2**32, (PHILOX_N_RANDOM, 6))]
    for nUE in (1, 100_000, 2**24):  # the shapes of real use
        for variant in range(4):
            ues = [0, nUE - 1, nUE // 2] + [int(v) for v in rng.integers(0, nUE, 60)] + [2**24 - 1]
            for ue in ues:
                for k in (0, 1, int(rng.integers(2, 200))):
                    seed = int(rng.integers(1, 2**32)) << 32 | int(rng.integers(0, 2**32))  # a 64-bit seed with a non-zero high half
                    rows.append((seed & U32, seed >> 32, ue, k, nUE, variant))
    a = np.array(rows, dtype=np.uint32)
    assert len(a) <= 20000
    return a


def philox_block(ob, ctr, key):
    out = (ctypes.c_uint32 * 4)()
    ob.lib().oracle_philox4x32_10((ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), out)
    return tuple(out)


def philox_reference(ob, cases):
    """(d, d1, d2) per case from the oracle's Philox block: the draw is word 0 >> 1.  _x2 draws at c1 and at (c1 + 1) mod 2^32 WITHOUT a carry into c2:
    the kernels' convention (the draw index of a UE is counter word 1 alone; prach_device_fn.h, philox_draw31_x2)."""
    ref = np.zeros((len(cases), 3), dtype=np.int64)
    for n, (k0, k1, c0, c1, c2, c3) in enumerate(cases.tolist()):
        d = philox_block(ob, (c0, c1, c2, c3), (k0, k1))[0] >> 1
        ref[n] = (d, d, philox_block(ob, (c0, (c1 + 1) & U32, c2, c3), (k0, k1))[0] >> 1)
    return ref


# ---- 2 masks ----------------------------------------------------------------------------------------------------------------------------------------------
MASK_T = (100, 60000)
MASK_MAXRAR = (1, 2, 5, 10)
MASK_MAXMSG2 = 10
MASK_PRE = (0, 1, 5, 255)
MASK_SAMPLE = 0.37  # the share of the enumeration the GPU test runs: 1.5 million records
GAP_WORD = 0xA5A5A5A5  # the arena's gap pattern (the engine's and the other harnesses' arenas fill their gaps with 0xA5 bytes)
FRONT_LANES = (0, 1, 31, 63, 64)


def enum_size(maxRar):
    return 7 * 7 * 2 * 6 * 3 * (maxRar + 2) * 4 * 3 * 4


def enum_decode(e, t, maxRar, consts):
    """The enumeration of the harness (prims_decode), restated in numpy: fields of record e of the class (t, maxRar)."""
    e = np.asarray(e, dtype=np.int64)
    f = {}
    krz, e = e % 7, e // 7
    krx, e = e % 7, e // 7
    f["grant"], e = e % 2, e // 2
    f["pend"], e = e % 6, e // 6
    kmrc, e = e % 3, e // 3
    f["rar"], e = e % (maxRar + 2), e // (maxRar + 2)
    kpre, e = e % 4, e // 4
    f["conn"], e = e % 3, e // 3
    f["act"] = e % 4
    f["rz"] = np.array([-2, 0, 1, t - 1, t, t + 1, t + 5], dtype=np.int64)[krz]
    f["rx"] = t - 4 + krx
    f["pre"] = np.array(MASK_PRE, dtype=np.int64)[kpre]
    f["mrc"] = np.where(kmrc == 0, 0, MASK_MAXMSG2 + kmrc - 1)
    f["pk"] = (f["act"] << consts["PK_ACT_SHIFT"]) | (f["conn"] << consts["PK_CONN_SHIFT"]) | (f["pre"] << consts["PK_PRE_SHIFT"]) | \
        (f["rar"] << consts["PK_RAR_SHIFT"]) | (f["mrc"] << consts["PK_MRC_SHIFT"]) | (f["pend"] << consts["PK_PEND_SHIFT"]) | (f["grant"] * consts["PK_GRANT_BIT"])
    # a PEND_STAY record was written at subframe rx <= t - 1 (its age is t - 1 - rx): the kernels never hold a younger one
    f["valid"] = ~((f["pend"] == consts["PEND_STAY"]) & (f["rx"] > t - 1))
    return f


def fields_of(pk, consts):
    pk = u32(pk)
    return dict(act=(pk >> consts["PK_ACT_SHIFT"]) & 3, conn=(pk >> consts["PK_CONN_SHIFT"]) & 3, pre=(pk >> consts["PK_PRE_SHIFT"]) & 0xff,
                rar=(pk >> consts["PK_RAR_SHIFT"]) & 0xff, mrc=(pk >> consts["PK_MRC_SHIFT"]) & 0xff, pend=(pk >> consts["PK_PEND_SHIFT"]) & 7,
                grant=(pk >> 31) & 1)


def light_predicate(pk, rx, rz, t, maxRar, consts, spec=False):
    """`light` as the comment above pass_masks states it: deferred outcome none / stay / caller without a grant, contending (Msg1 phase, a preamble chosen,
    backoff run out), and the RAR window stays open after this subframe, where a PEND_STAY record has aged t - 1 - rx subframes.  SPEC: not a new caller."""
    f = fields_of(pk, consts)
    age = np.where(f["pend"] == consts["PEND_STAY"], t - 1 - np.asarray(rx, dtype=np.int64), 0)
    ok = (f["pend"] <= 2) & (f["grant"] == 0) & (f["act"] == consts["ACT_M1"]) & (f["pre"] != 0) & (np.asarray(rz, dtype=np.int64) <= t) & (f["rar"] + age + 1 < maxRar)
    if spec:
        ok &= f["pend"] != consts["PEND_CALLER"]
    return ok


class MaskCases:
    """groups[ng][8] = t, maxRar, front, i0, acNow, acPrev, nUE, 0; recs[n][4] = kind, a, b, c; twin[g]: for a front group, the group that holds the same
    records without a front (-1 otherwise)."""


def _mask_class_indices(t, maxRar, consts, full):
    n = enum_size(maxRar)
    e = np.arange(n, dtype=np.int64)
    e = e[enum_decode(e, t, maxRar, consts)["valid"]]
    e = e[np.random.default_rng(1000 * maxRar + t).permutation(len(e))]  # a wavefront mixes classes
    if full:
        return np.concatenate([e, e[:(-len(e)) % 64]])
    return e[:int(len(e) * MASK_SAMPLE) // 64 * 64]


def mask_cases(consts, full=False, front=True):
    """full: every valid record of the enumeration (the CPU test); else a fixed-seed sample of it.  front: the arrival-front groups and their twins."""
    groups, recs = [], []
    for t in MASK_T:
        for maxRar in MASK_MAXRAR:
            e = _mask_class_indices(t, maxRar, consts, full)
            ng = len(e) // 64
            g = np.zeros((ng, 8), dtype=np.int64)
            g[:, 0], g[:, 1], g[:, 3] = t, maxRar, 64 * (np.arange(ng) % 4096)
            g[:, 4:7] = 1 << 22
            r = np.zeros((len(e), 4), dtype=np.int64)
            r[:, 1] = e
            groups.append(g)
            recs.append(r)
    M = MaskCases()
    nplain = sum(len(g) for g in groups)
    twin = [-1] * nplain
    if front:
        rng = np.random.default_rng(2)
        fg, fr = [], []
        for t, maxRar in ((100, 5), (60000, 10), (100, 2)):
            e = np.arange(enum_size(maxRar), dtype=np.int64)
            f = enum_decode(e, t, maxRar, consts)
            light = light_predicate(f["pk"], f["rx"], f["rz"], t, maxRar, consts) & f["valid"]
            idle = (f["pend"] == 0) & (f["grant"] == 0) & (f["act"] <= 1) & f["valid"]
            pools = (e[light], e[idle], e[f["valid"]])
            for a in FRONT_LANES:
                for b in FRONT_LANES:
                    for c in FRONT_LANES:
                        if not a <= b <= c:
                            continue
                        for fill in ("gap", "random"):
                            i0 = 64 * int(rng.integers(1, 1000))
                            r = np.zeros((64, 4), dtype=np.int64)
                            for lane in range(64):
                                if lane < b:
                                    if a <= lane and lane % 4 == 3:
                                        r[lane] = (1, 0, 0, 0)  # what the kernels hold for a UE that has not arrived: an all-zero record
                                    else:
                                        pool = pools[lane % 3]
                                        r[lane] = (0, int(pool[rng.integers(0, len(pool))]), 0, 0)
                                else:
                                    r[lane] = (1,) + ((GAP_WORD,) * 3 if fill == "gap" else tuple(int(v) for v in rng.integers(0, 2**32, 3)))
                            for is_front in (1, 0):
                                fg.append((t, maxRar, is_front, i0, i0 + b, i0 + a, i0 + c, 0))
                                fr.append(r)
                            twin += [nplain + len(fg) - 1, -1]
        groups.append(np.array(fg, dtype=np.int64))
        recs.append(np.concatenate(fr))
    M.groups, M.recs, M.twin = np.concatenate(groups), np.concatenate(recs), np.array(twin)
    M.nplain = nplain
    M.n = len(M.recs)
    assert M.n == 64 * len(M.groups) == 64 * len(M.twin)
    return M


def write_masks(path, M):
    write_case(path, "masks", M.n, [M.groups, M.recs], p3=MASK_MAXMSG2)


class MaskTable:
    """The branched body's answer for every record of a case file (`--host`), and what the tests need of it per record."""

    def __init__(self, M, host_words, consts):
        w = host_words.reshape(M.n, 8).astype(np.int64)
        c = consts
        self.t = np.repeat(M.groups[:, 0], 64)
        self.maxRar = np.repeat(M.groups[:, 1], 64)
        flags, ntx, nbo, npk, ntb = w[:, 0], as_i32(w[:, 1]), as_i32(w[:, 2]), w[:, 3], as_i32(w[:, 7])
        self.rx, self.rz, self.pk = as_i32(w[:, 4]), as_i32(w[:, 5]), w[:, 6]
        f = fields_of(self.pk, c)
        self.f = f
        t = self.t
        tb0 = t - c["PRIMS_TB_BACK"]
        self.applied, self.dirty, self.need, self.evtype = flags & 1, (flags >> 1) & 1, (flags >> 2) & 3, (flags >> 4) & 7
        untouched = ((flags >> 7) & 3) == 0  # cold fields and counters
        # a no-op: ue_apply returned false, no draw, not dirty, no event, state, cold fields and counters untouched
        self.noop = (flags == 0) & (ntx == self.rx) & (nbo == self.rz) & (npk == self.pk) & (ntb == tb0)
        # the light path of phase A (prach_cluster.hip compact_phase_a, prach_lcluster.hip): rar++ on the aged record, the bump, PEND_STAY for a member
        age = np.where(f["pend"] == c["PEND_STAY"], t - 1 - self.rx, 0)
        had = f["pend"] != c["PEND_NONE"]
        want_pend = np.where(had | (self.rx == t), c["PEND_STAY"], c["PEND_NONE"])
        want_pk = (f["act"] << c["PK_ACT_SHIFT"]) | (f["conn"] << c["PK_CONN_SHIFT"]) | (f["pre"] << c["PK_PRE_SHIFT"]) | \
            (((f["rar"] + age + 1) & 0xff) << c["PK_RAR_SHIFT"]) | (f["mrc"] << c["PK_MRC_SHIFT"]) | (want_pend << c["PK_PEND_SHIFT"])
        self.light_state = (self.need == 0) & (self.evtype == c["UEV_NONE"]) & untouched & (ntx == np.where(had, t, self.rx)) & (nbo == self.rz) & (ntb == tb0) & \
            (npk == want_pk)
        self.pred = light_predicate(self.pk, self.rx, self.rz, t, self.maxRar, c)
        self.pred_spec = light_predicate(self.pk, self.rx, self.rz, t, self.maxRar, c, spec=True)
        self.trig = self.rx == t
        self.done = f["act"] == c["ACT_DONE"]


# ---- 3 wave -----------------------------------------------------------------------------------------------------------------------------------------------
WAVE_N_RANDOM = 300


def wave_cases():
    """[(name, row[64] int64 in int32 range)]"""
    rng = np.random.default_rng(3)
    cases = []
    for k in range(64):
        r = np.zeros(64, dtype=np.int64)
        r[k] = 1 + 1000 * k  # (a value of its own per lane: who reached whom shows in the sum)
        cases.append((f"one_hot_{k}", r))
    cases.append(("all_ones", np.ones(64, dtype=np.int64)))
    cases.append(("lane_index", np.arange(64, dtype=np.int64)))
    cases.append(("negative", -1 - 3 * np.arange(64, dtype=np.int64)))
    cases.append(("mixed_sign", (np.arange(64, dtype=np.int64) - 31) * 1_000_003))
    cases.append(("sum_wraps_2_31", np.full(64, 2**26 + 12345, dtype=np.int64)))
    cases.append(("sum_wraps_2_31_in_row_1", np.where(np.arange(64) < 20, 2**27 - 1, 7)))
    cases.append(("sum_wraps_2_32", np.full(64, INT_MAX, dtype=np.int64)))
    cases.append(("sum_wraps_negative", np.full(64, INT_MIN, dtype=np.int64)))
    for k in range(64):
        r = np.full(64, INT_MIN, dtype=np.int64)
        r[k] = -5 + k
        cases.append((f"max_in_lane_{k}_int_min_elsewhere", r))
        r = rng.integers(-2**30, 1000, 64)
        r[k] = 1000 + k
        cases.append((f"max_in_lane_{k}_smaller_elsewhere", r))
    cases.append(("all_int_min", np.full(64, INT_MIN, dtype=np.int64)))
    cases.append(("rows_count_2_1_0", np.repeat(np.array([2, 1, 0, 2]), 16)))
    for k in range(WAVE_N_RANDOM):
        lo, hi = ((INT_MIN, INT_MAX + 1), (-2**20, 2**20), (0, 3))[k % 3]
        cases.append((f"random_{k:03d}", rng.integers(lo, hi, 64)))
    return cases


def wave_reference(rows):
    """scan, sum (mod 2^32), max per row, in int64."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.cumsum(rows, axis=1) & U32, rows.sum(axis=1) & U32, rows.max(axis=1) & U32


# ---- 4 mod ------------------------------------------------------------------------------------------------------------------------------------------------
MOD_DIVISORS = tuple(range(1, 257)) + (1000, 54321, 2**16 - 1, 2**16 + 1, 2**20, 2**31 - 1)
MOD_N_RANDOM = 300


def mod_cases():
    """rows of (x, d, sub, aT): x any uint32, 1 <= d < 2^31, sub >= 0, aT 1..20 (the accessTime m of Beta.c:268-277 is taken from)."""
    rng = np.random.default_rng(4)
    rows = []
    for n, d in enumerate(MOD_DIVISORS):
        xs = [0, 1, d - 1, d, d + 1, 2**31 - 1, 2**31, 2**32 - 1]
        for lim in (2**31, 2**32):
            k = (lim - 1) // d  # the largest k with k d below the limit
            xs += [k * d - 1, k * d, k * d + 1]
        xs = [x for x in xs if 0 <= x < 2**32] + [int(v) for v in rng.integers(0, 2**32, MOD_N_RANDOM)]
        for j, x in enumerate(xs):
            aT = 1 + (n + j) % 20
            sub = x if x <= INT_MAX - 32 else x % (INT_MAX - 32)
            rows.append((x, d, sub, aT))
    for aT in range(1, 21):  # every residue of every accessTime, at both ends of the range
        for base in (0, 60000, INT_MAX - 32 - 2 * aT):
            rows += [(base + m, aT, base + m, aT) for m in range(2 * aT)]
    return np.array(rows, dtype=np.int64)


def slot_align_py(sub, aT):  # Beta.c:268-277
    m = sub % aT
    return sub + 1 if m == 0 else (sub if m == 1 else sub + (aT - m + 1))


def mod_reference(cases):
    """x % d on the value as unsigned 32-bit, and the three-line definition of slot_align."""
    x, d, sub, aT = (cases[:, k] for k in range(4))
    return x % d, np.array([slot_align_py(int(s), int(a)) for s, a in zip(sub, aT)], dtype=np.int64)


# ---- 5 sector ---------------------------------------------------------------------------------------------------------------------------------------------
def sector_reference(d):
    """activateUEs (WithNOMA:393-410) in numpy float32 operations, compared with the double constants k / 3 * (double)3.14f and 3.14."""
    f = np.float32
    pi = f(3.14)
    theta = (np.asarray(d, dtype=np.int64).astype(f) / f(2147483647)) * f(2) * pi
    assert theta.dtype == np.float32
    th, pid = theta.astype(np.float64), np.float64(pi)
    out = np.full(th.shape, 5, dtype=np.int64)
    conds = [(th >= 0) & (th < (1. / 3.) * pid), (th >= (1. / 3.) * pid) & (th < (2. / 3.) * pid), (th >= (2. / 3.) * pid) & (th < 3.14),
             (theta >= pi) & (th < (4. / 3.) * pid), (th >= (4. / 3.) * pid) & (th < (5. / 3.) * pid)]
    for k in range(4, -1, -1):
        out = np.where(conds[k], k, out)
    return out


def sector_boundaries():
    """For k = 1..5 the first draw whose sector is >= k (bisection in the numpy statement)."""
    out = []
    for k in range(1, 6):
        lo, hi = 0, INT_MAX
        assert sector_reference(lo) < k <= sector_reference(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if sector_reference(mid) >= k:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return out


def sector_cases():
    rng = np.random.default_rng(5)
    d = [0, 1, INT_MAX] + list(range(2**31 - 64, 2**31))
    for b in sector_boundaries():
        d += list(range(b - 64, b + 64))
    d += [int(v) for v in rng.integers(0, 2**31, 4000)]
    return np.array(d, dtype=np.int64)


# ---- 6 granule --------------------------------------------------------------------------------------------------------------------------------------------
def granule_cases(consts):
    """rows of (kind, a, b, tag, probe).  kind 0: mk_granule(a, b, tag); kind 1: the words a, b as they are.  The granule must be ok under `tag` (kind 0)
    and not ok under `probe` (every row's probe differs from its tag in the 16 bits a tag has)."""
    rng = np.random.default_rng(6)
    V = np.array([0, 1, 0x7FFFF, 0xFFFFE, consts["GR_NONE"]], dtype=np.int64)
    tags = np.arange(0x10000, dtype=np.int64)
    rows = []
    # every tag with five of the 25 value pairs (all 25 over any five consecutive tags), probed with each kind of wrong tag in turn
    probes = [lambda t: t + 1, lambda t: t - 1, lambda t: t + 0x1000, lambda t: t - 0x1000, lambda t: t ^ 0x8000, lambda t: t - 2]  # t - 2: the stale granule of the
    for j in range(5):                                                                                                               # same parity's previous subframe
        for q, probe in enumerate(probes):
            sel = tags[tags % 6 == (q + j) % 6]
            rows.append(np.stack([np.zeros_like(sel), np.full(len(sel), V[j]), V[(j + sel) % 5], sel, probe(sel) & 0xFFFF], axis=1))
    # 32-bit inputs: nothing above bit 19 may reach the tag bits
    wide = rng.integers(0, 2**32, (4000, 2))
    wide[:200] |= 0xFFF00000
    wide[200:400] = U32
    t = rng.integers(0, 0x10000, 4000)
    rows.append(np.stack([np.zeros(4000, dtype=np.int64), wide[:, 0], wide[:, 1], t, (t + 1 + rng.integers(0, 0xFFFF, 4000)) & 0xFFFF], axis=1))
    # an all-zero and an all-ones word are no granule of subframe 0 (tag 1) or of the last one (tag 60 001)
    for w in (0, U32):
        for tag in (1, 60001):
            rows.append(np.array([[1, w, w, tag, tag]], dtype=np.int64))
    return np.concatenate(rows)


def granule_reference(cases):
    """Python integer bit-slicing: words of a made granule, and whether a granule's 12 + 4 tag bits equal a tag's low 16 bits."""
    kind, a, b, tag, probe = (cases[:, k] for k in range(5))
    w0 = np.where(kind == 0, (a & 0xFFFFF) | ((tag & 0xFFF) << 20), a)
    w1 = np.where(kind == 0, (b & 0xFFFFF) | (((tag >> 12) & 0xF) << 20), b)
    carried = (w0 >> 20) | (((w1 >> 20) & 0xF) << 12)
    return w0, w1, carried == (tag & 0xFFFF), carried == (probe & 0xFFFF)


# ---- 7 blocks ---------------------------------------------------------------------------------------------------------------------------------------------
BLOCK_G = (1, 2, 3, 8, 32, 64)
BLOCK_NTRIALS = (1, 7, 8, 9, 16, 17, 1000)


def launch_grid(G, xpack, ntrials):
    """The grid of launch_lcluster_kernel / launch_noma_kernel, restated (tests/test_prims_cases_cpu.py holds it against their source lines)."""
    return (ntrials + 7) // 8 * 8 * G if xpack else ntrials * G


def block_sets():
    return np.array([(G, x, n, launch_grid(G, x, n)) for G in BLOCK_G for x in (0, 1) for n in BLOCK_NTRIALS], dtype=np.int64)


def launcher_grid_expressions():
    """{file: the C expression `grid` is initialised with in its launcher}"""
    out = {}
    for name in ("prach_lcluster.hip", "prach_noma.hip"):
        with open(os.path.join(CSRC, name)) as f:
            m = re.findall(r"const int grid = ([^;]+);", f.read())
        assert len(m) == 1, (name, m)
        out[name] = m[0]
    return out


def eval_c_grid(expr, G, xpack, ntrials):
    """cond ? a : b over + * / ( ) of non-negative ints."""
    m = re.fullmatch(r"\s*(\w+)\s*\?\s*(.+?)\s*:\s*(.+?)\s*", expr)
    assert m and re.fullmatch(r"[\w\s+*/()]+", m.group(2) + m.group(3)), expr
    env = dict(G=G, xpack=xpack, ntrials=ntrials)
    return eval((m.group(2) if env[m.group(1)] else m.group(3)).replace("/", "//"), {"__builtins__": {}}, env)


# ---- 8 hot ------------------------------------------------------------------------------------------------------------------------------------------------
def hot_cases(consts):
    """rows of (tx, bo, pk, fits)"""
    rng = np.random.default_rng(8)
    B = consts["HOT_BO_BIAS"]
    txs, bos = (-1, 0, 1, 65533, 65534), (-B, -1, 0, 1, 65535 - B)
    rows = [(tx, bo, int(pk), 1) for tx in txs for bo in bos for pk in np.concatenate([rng.integers(0, 2**32, 6), rng.integers(2**31, 2**32, 2)])]
    for tx in (-2, 65535):  # the first value outside each bound
        rows += [(tx, bo, int(rng.integers(0, 2**32)), 0) for bo in bos]
    for bo in (-B - 1, 65536 - B):
        rows += [(tx, bo, int(rng.integers(0, 2**32)), 0) for tx in txs]
    return np.array(rows, dtype=np.int64)


def slot_pairs(consts):
    return np.array([(G, b) for G in range(1, consts["CLUSTER_MAX_G"] + 1) for b in range(G)], dtype=np.int64)


def idx_of_reference(pairs, lslots):
    """Ownership is interleaved (prach_cluster.hip): 64-UE group g belongs to workgroup g % G, so local group j of workgroup b is group b + G j, and slot
    64 j + lane holds UE 64 (b + G j) + lane."""
    slot = np.arange(lslots, dtype=np.int64)[None, :]
    G, b = pairs[:, 0][:, None], pairs[:, 1][:, None]
    return (b + G * (slot // 64)) * 64 + slot % 64


# ---- 9 pack -----------------------------------------------------------------------------------------------------------------------------------------------
def pack_cases():
    rng = np.random.default_rng(9)
    r = rng.integers(0, 2**32, (3000, 4))
    r[:8, 3] = [0, U32, 0x7FFFFFFF, 0x80000000, 0x0FFFFFFF, 0x70000000, 0x000FF000, 0x00000FF3]
    return r
