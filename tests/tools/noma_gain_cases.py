"""The two kernels of prach_noma_gain.hip away from the engine: seeded cases of per-UE state, levels and ln(gain) values no NOMA.c trial leaves behind, with the
numpy restatement of tests/tools/noma_gain_ref.py as their reference, and the glue around tests/tools/gpu_noma_gain_harness.hip (case file, side file, result
file, one child process per launch).  Shared by tests/test_noma_gain_cases_cpu.py and tests/test_gpu_noma_gain_synthetic.py.

REDUCER CASES (crafted records and LEVELS): UEs of every class and STATE, sectors outside 0..5, negative SOJOURN / TIMER / PTC words (noma_census_cases.wild_logs
and noma_timeline_cases.wild); levels exactly on lo, on lo + bins * width - 1, on every inner edge, one below, one above, and INT32_MIN; bins 1, 2, 4096 and the
two sizes around the LDS limit; width 1 and 2^20; lo at INT32_MIN + 1 and at a positive value; sums past 2^32 in one cell, addends on and above the 32-bit tile
budget; nUE of 1, tile - 1, tile, tile + 1 and three tiles; 300 jobs into 3 groups.
LEVEL CASES (crafted ln(gain)): products inside the band on both sides of an integer and exactly on it, just outside the band, no level (NaN, infinities,
2^30), a level outside the range the band is derived for, ordinary values — and a list one entry shorter than the EDGE UEs.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import noma_census_cases as NC
import noma_census_ref as N
import noma_gain_ref as G
import noma_timeline_cases as TC
import reduce_cases as R

TILE = R.TILE
LDS_MAX_BINS, MAX_ADDEND, EDGE_CAP, BAND, RANGE = 511, 10006, 4096, 1e-8, 32768.0
CONSTANTS = dict(TL_TILE=8192, TL_THREADS=256, TILE_SCHED_CAP=2048, NG_SCALARS=16, NG_EDGE_CAP=EDGE_CAP, NG_LDS_MAX_BINS=LDS_MAX_BINS, NG_MAX_ADDEND=MAX_ADDEND,
                 NG_LEVEL_BAND=BAND, NG_LEVEL_RANGE=RANGE)
NG_SCALARS, KIND, GUARD, PATTERN = 16, 14, 64, 0x7FFF7FFF
HARNESS = "gpu_noma_gain_harness.hip"
SIZES = (1, TILE - 1, TILE, TILE + 1, 3 * TILE)
NOMA_KW = NC.NOMA_KW
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


class Job(NC.Job):
    """A NOMA job (records, schedule, E) plus the per-UE levels and ln(gain) values."""

    def __init__(self, logs, sched, access_time, group, E, level, cfg_kw=None, lgain=None):
        super().__init__(logs, sched, access_time, group, E, cfg_kw)
        self.level = np.ascontiguousarray(level, dtype=np.int32)
        self.lgain = np.zeros(self.nue, dtype=np.float64) if lgain is None else np.ascontiguousarray(lgain, dtype=np.float64)
        assert self.level.shape == (self.nue,) and self.lgain.shape == (self.nue,)


class Case:
    """host: every schedule is the product's own NOMA.c schedule, so the host definition (prach_noma_gain_accumulate_levels) applies."""

    def __init__(self, name, bins, width, lo, ngroups, jobs, host):
        self.name, self.bins, self.width, self.lo, self.ngroups, self.jobs, self.host = name, int(bins), int(width), int(lo), int(ngroups), jobs, host

    def __repr__(self):
        return self.name

    def reference(self):
        return G.profile([j.logs for j in self.jobs], [j.sched for j in self.jobs], [j.access_time for j in self.jobs], [j.E for j in self.jobs],
                         [j.level for j in self.jobs], self.bins, self.width, self.lo, groups=[j.group for j in self.jobs], ngroups=self.ngroups)

    def host_definition(self, pkg):
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        t = pkg.noma_gain_from_levels(cfgs, [j.E for j in self.jobs], [j.logs for j in self.jobs], [j.level for j in self.jobs], self.bins, self.width, self.lo,
                                      groups=[j.group for j in self.jobs], ngroups=self.ngroups)
        return {"series": t.series.astype(np.int64), "scalars": t.scalars}


CASE_NAMES = ("sizes_wild_records", "edges_bins2", "bins1_width_2p20_lo_int_min", "bins4096_width1_positive_lo", "lds_limit_bins511", "lds_limit_bins512",
              "budget_addends_and_sums_past_2p32", "jobs_300_groups_3")


def _levels(rng, n, lo, hi, special):
    """Levels drawn over [lo - margin, hi + margin) with the `special` ones sprinkled in (every one of them at least once where n allows)."""
    span = max(hi - lo, 1)
    L = rng.integers(lo - span // 8 - 2, hi + span // 8 + 2, n).astype(np.int64)
    L = np.clip(L, INT_MIN + 1, INT_MAX)
    at = rng.permutation(n)[:min(n, 3 * len(special))]
    L[at] = np.resize(np.asarray(special, dtype=np.int64), len(at))
    return L


def _real_jobs(pkg, rng, groups, lo, hi, special, sizes=SIZES):
    """The product's NOMA.c schedule, E inside the arrivals for every third job and at maxTime otherwise; wild records."""
    jobs = []
    for n in sizes:
        sched = pkg.arrival_schedule(pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **NOMA_KW))[0]
        at = R.arrival_times(n, sched, NOMA_KW["accessTime"])
        E = int(at[n // 2]) if len(jobs) % 3 == 0 else 10000
        jobs.append(Job(TC.wild(rng, at, E), sched, NOMA_KW["accessTime"], len(jobs) % groups, E, _levels(rng, n, lo, hi, special), dict(NOMA_KW)))
    return jobs


def _edge_levels(bins, width, lo):
    hi = lo + bins * width
    inner = [lo + b * width for b in range(1, bins)] if bins <= 64 else [lo + width, lo + (bins // 2) * width, lo + (bins - 1) * width]
    return [lo, hi - 1, lo - 1, hi, INT_MIN] + inner + [e - 1 for e in inner]


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    for name, bins, width, lo, seed, sizes in (("sizes_wild_records", 65, 200, -16200, 1400, SIZES), ("edges_bins2", 2, 7, -50, 1401, (65, TILE + 1)),
                                               ("bins1_width_2p20_lo_int_min", 1, 2 ** 20, INT_MIN + 1, 1402, (65, TILE + 1)),
                                               ("bins4096_width1_positive_lo", 4096, 1, 1000, 1403, (TILE + 1,)),
                                               ("lds_limit_bins511", LDS_MAX_BINS, 25, -16200, 1404, (TILE + 1,)),
                                               ("lds_limit_bins512", LDS_MAX_BINS + 1, 25, -16200, 1405, (TILE + 1,))):
        hi = lo + bins * width
        special = [v for v in _edge_levels(bins, width, lo) + [0, INT_MAX, INT_MIN + 1] if INT_MIN <= v <= INT_MAX]
        ng = min(len(sizes), 4)
        out.append(Case(name, bins, width, lo, ng, _real_jobs(pkg, np.random.default_rng(seed), ng, lo, hi, special, sizes), True))

    # addends of exactly the 32-bit tile budget and one above, alone and together, and three preamble counts of INT_MAX in ONE cell (its sum is past 2^32), in
    # two tiles of ordinary served UEs that all sit in two cells: the product's schedule, so the host definition applies
    rng = np.random.default_rng(1410)
    n = 2 * TILE + 3
    sched = pkg.arrival_schedule(pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **NOMA_KW))[0]
    at = R.arrival_times(n, sched, NOMA_KW["accessTime"])
    soj, tim, ptc = rng.integers(0, 3000, n), rng.integers(0, 3000, n), rng.integers(0, 12, n)
    tim = np.minimum(tim, soj)
    for k, (s, t, p) in enumerate(((MAX_ADDEND, 0, 1), (MAX_ADDEND + 1, 0, 1), (MAX_ADDEND + 1, MAX_ADDEND + 1, 1), (5, 0, MAX_ADDEND), (5, 0, MAX_ADDEND + 1),
                                   (5, 5, INT_MAX), (6, 0, INT_MAX), (7, 7, INT_MAX), (INT_MAX - 20000, 3, 2))):
        soj[100 * k + 7], tim[100 * k + 7], ptc[100 * k + 7] = s, t, p
    a = TC.served(n, at, soj, tim, 3)
    a[:, N.W_PTC] = ptc
    L = np.where(np.arange(n) % 5 == 0, -9000, -8800)
    out.append(Case("budget_addends_and_sums_past_2p32", 65, 200, -16200, 1, [Job(a, sched, NOMA_KW["accessTime"], 0, 10000, L, dict(NOMA_KW))], True))

    # 300 jobs into 3 groups, synthetic schedules
    rng = np.random.default_rng(1420)
    jobs = []
    for k in range(300):
        n = int(rng.integers(1, 41))
        nslots = int(rng.integers(1, 60))
        sched = R.sched_from_slots(np.sort(rng.integers(0, nslots + 1, n)), nslots)
        jobs.append(Job(TC.wild(rng, R.arrival_times(n, sched, 5), 5 * nslots), sched, 5, int(rng.integers(0, 3)), 5 * nslots, _levels(rng, n, -16200, -3200, [INT_MIN, -16200, -3201])))
    out.append(Case("jobs_300_groups_3", 65, 200, -16200, 3, jobs, False))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the level pre-pass -------------------------------------------------------------------------------------------------------------------------------

def product_of(lgain):
    """1000.0 * lgain, one float64 multiplication, as float64."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float64(1000.0) * np.asarray(lgain, dtype=np.float64)


def edge_of(lgain, band=BAND, rng_limit=RANGE):
    """Whether the pre-pass must list the UE: no level, a product outside the range the band is derived for, or within the band of an integer."""
    p = product_of(lgain)
    has = np.isfinite(p) & (np.abs(p) < 2.0 ** 30)
    with np.errstate(invalid="ignore"):
        d = p - np.floor(p)
        return ~has | ~(np.abs(p) < rng_limit) | (d <= band) | (d >= 1.0 - band)


class LevelCase:
    """jobs of ln(gain) values; `inside` / `outside`: (job, UE) pairs placed inside / just outside the band by construction; cap: the list's capacity."""

    def __init__(self, name, lgains, inside, outside, cap):
        self.name, self.inside, self.outside, self.cap = name, set(inside), set(outside), int(cap)
        self.jobs = [Job(np.zeros((len(lg), 16), dtype=np.int32), np.array([len(lg)], dtype=np.int32), 5, 0, 0, np.zeros(len(lg), dtype=np.int32), None, lg) for lg in lgains]
        self.bins, self.width, self.lo, self.ngroups = 1, 1, 0, 1

    def __repr__(self):
        return self.name

    def expected_levels(self):
        return np.concatenate([G.level_of(j.lgain) for j in self.jobs])

    def expected_edges(self):
        return {(k, int(i)) for k, j in enumerate(self.jobs) for i in np.flatnonzero(edge_of(j.lgain))}


LEVEL_CASE_NAMES = ("band_sides_three_jobs", "one_more_than_the_list_holds")


def _band_job(rng, n, k0):
    """n ordinary ln(gain) values of a trial's range; then, at known places: products inside the band below, on and above an integer, and just outside it on
    both sides; no level; a level outside the derived range."""
    lg = rng.uniform(-16.1, -3.36, n)
    inside, outside = [], []
    where = iter(rng.permutation(n))
    for q, k in enumerate(range(k0, k0 + 6)):
        for off, into in ((-0.4e-8, inside), (0.4e-8, inside), (0.0, inside), (-3e-8, outside), (3e-8, outside), (0.5, outside)):
            i = int(next(where, -1))
            if i < 0:
                break
            lg[i] = (-1000.0 * (q + 4) - k + off) / 1000.0
            into.append(i)
    for v in (np.nan, np.inf, -np.inf, 2.0 ** 30 / 1000.0, -2.0 ** 30 / 1000.0, 40.5004, -33.0001):
        i = int(next(where, -1))
        if i >= 0:
            lg[i] = v
            inside.append(i)
    return lg, inside, outside


def level_cases():
    out = []
    rng = np.random.default_rng(1450)
    lgs, inside, outside = [], [], []
    for k, n in enumerate((1, TILE + 1, 70)):
        lg, i, o = _band_job(rng, n, 100 * k + 3)
        lgs.append(lg)
        inside += [(k, x) for x in i]
        outside += [(k, x) for x in o]
    out.append(LevelCase("band_sides_three_jobs", lgs, inside, outside, EDGE_CAP))
    # nine EDGE UEs, a list of eight
    lg = rng.uniform(-16.1, -3.36, TILE + 5)
    lg[edge_of(lg)] = -7.5005
    at = rng.permutation(len(lg))[:9]
    lg[at] = -(5.0 + np.arange(9))  # products exactly on an integer
    out.append(LevelCase("one_more_than_the_list_holds", [lg], [(0, int(i)) for i in at], [], 8))
    assert tuple(c.name for c in out) == LEVEL_CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    """The case file and, next to it, the side file (path + ".side"): float64 lgain of every UE in job order, then int32 levels."""
    head = np.zeros(16, dtype=np.int32)
    head[:7] = [R.MAGIC, KIND, len(case.jobs), case.bins, case.width, case.lo, case.ngroups]
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group, j.E]))
    with open(path + ".side", "wb") as f:
        f.write(np.concatenate([j.lgain for j in case.jobs]).astype("<f8").tobytes())
        f.write(np.concatenate([j.level for j in case.jobs]).astype("<i4").tobytes())


def _header(case, raw, mode):
    wgs = sum(-(-j.nue // TILE) for j in case.jobs)
    head = np.frombuffer(raw[:32], dtype="<u8")
    assert [int(v) for v in head] == [R.MAGIC, KIND, mode, wgs], head


def read_result(case, path, scheme):
    """The reducer's result as {"series", "scalars"}; trials and ues are the host's own count, as in the engine."""
    raw = open(path, "rb").read()
    _header(case, raw, scheme)
    r = np.frombuffer(raw[32:], dtype="<u8")
    ng, bins = case.ngroups, case.bins
    assert r.size == 36 * ng * bins + ng * NG_SCALARS
    out = G.empty(ng, bins)
    out["series"][:] = r[:36 * ng * bins].reshape(6, ng, 6, bins).astype(np.int64)
    sc = r[36 * ng * bins:].reshape(ng, NG_SCALARS).astype(np.int64)
    for q, f in enumerate(("idle", "served", "dropped", "pending", "undefined", "below", "above", "restarted", "sojourn_sum", "lost_sum", "ptc_sum", "defined")):
        out["scalars"][f][:] = sc[:, q]
    has = sc[:, 11] > 0
    out["scalars"]["level_max"][:] = np.where(has, sc[:, 12] - 2 ** 31, -1)
    out["scalars"]["neg_level_max"][:] = np.where(has, sc[:, 13] - 2 ** 31, -1)
    assert not sc[:, 14:].any() and not sc[~has, 12:14].any()
    for j in case.jobs:
        out["scalars"]["trials"][j.group] += 1
        out["scalars"]["ues"][j.group] += j.nue
    return out


def read_levels(case, path):
    """The pre-pass's result: (count, listed (job, UE) pairs in list order, the words behind the list, the level column int64 [total UEs])."""
    raw = open(path, "rb").read()
    _header(case, raw, 2)
    total = sum(j.nue for j in case.jobs)
    w = np.frombuffer(raw[32:], dtype="<u4")
    nlist = 2 + 2 * case.cap
    assert w.size == nlist + GUARD + total
    count = int(w[0])
    assert int(w[1]) == 0
    stored = min(count, case.cap)
    pairs = [(int(w[2 + 2 * q]), int(w[3 + 2 * q])) for q in range(stored)]
    assert not w[2 + 2 * stored:nlist].any()  # the entries nobody took are still zero
    return count, pairs, w[nlist:nlist + GUARD].copy(), w[nlist + GUARD:].view("<i4").astype(np.int64)


def run_harness(exe, case, case_path, mode, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run): mode 0 / 1 the reducer under that scheme, 2 the level pre-pass."""
    res = os.path.join(str(out_dir), f"{case.name}.m{mode}.result")
    H.run(exe, [case_path, res, mode, case_path + ".side"] + ([case.cap] if mode == 2 else []), timeout)
    return read_levels(case, res) if mode == 2 else read_result(case, res, mode)
