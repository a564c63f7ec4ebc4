"""The two on-device reductions (prach::dist_kernel, prach::timeline_kernel) away from the engine: numpy references in int64 / Python ints, a
deterministic generator of synthetic per-UE state that no simulation leaves behind, and the glue around tests/tools/gpu_reduce_harness.hip (case file,
result file, one child process per launch).  Shared by tests/test_reduce_cases_cpu.py, tests/test_gpu_reduce_synthetic.py, tests/test_gpu_dist.py
(bincount_dist) and tests/tools/timeline_ref.py (timeline_add).  No GPU and no package import here: what needs the package takes it as an argument."""
import os

import numpy as np

import harness as H
from harness import constants as harness_constants  # noqa: F401  (the tests of the families built on this module reach it through here)

INT_MIN, INT_MAX = -2**31, 2**31 - 1
TIMER, ACTIVE, TXTIME, PTC, FLAG = 1, 2, 3, 11, 14  # columns of the 16-field per-UE log
# compile-time constants of the kernels (prach_device.h, prach_timeline.hip); tests/test_reduce_cases_cpu.py holds them against `gpu_reduce_harness --constants`
CONSTANTS = dict(DIST_TILE=8192, DIST_THREADS=256, DIST_PTC_BINS=256, DIST_SCALARS=8, TL_TILE=8192, TL_THREADS=256, TL_WINDOW=2048, TL_MAX_SOJOURN=60006,
                 TL_SCHED_CAP=2048, TL_SCALARS=8)
TILE, PTC_BINS, WINDOW, MAX_SOJOURN, SCHED_CAP = 8192, 256, 2048, 60006, 2048
DIST_FIELDS = ("trials", "ues", "success", "delay_overflow", "delay_sum", "ptc_sum", "delay_max")
TL_SERIES = ("arrivals", "success", "sojourn_sum", "timer_sum", "done")
TL_FIELDS = ("trials", "ues", "arrived", "success", "restarted", "arrival_overflow", "done_overflow", "sojourn_sum", "timer_sum", "done_max")
MAGIC = 0x52445543
HARNESS = "gpu_reduce_harness.hip"
PATTERN = 0x7FFF7FFF  # fills what no reduction may read: as a count or a time it would show in every output


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------

class RefDist:
    """The shape of the package's Dist (delay_hist, ptc_hist, one int64 array per field of DIST_FIELDS) without the package."""

    def __init__(self, ngroups, delay_bins, delay_bin_ms=1):
        self.delay_bins, self.delay_bin_ms, self.ngroups = int(delay_bins), int(delay_bin_ms), int(ngroups)
        self.delay_hist = np.zeros((self.ngroups, self.delay_bins), dtype=np.uint64)
        self.ptc_hist = np.zeros((self.ngroups, PTC_BINS), dtype=np.uint64)
        for f in DIST_FIELDS:
            setattr(self, f, np.zeros(self.ngroups, dtype=np.int64))
        self.delay_max[:] = -1


class RefTimeline:
    """The shape of the package's Timeline (series[name] [ngroups, bins] uint64, scalars[field] int64) without the package."""

    def __init__(self, ngroups, bins, bin_ms=1):
        self.bins, self.bin_ms, self.ngroups = int(bins), int(bin_ms), int(ngroups)
        self.series = {n: np.zeros((self.ngroups, self.bins), dtype=np.uint64) for n in TL_SERIES}
        self.scalars = {f: np.zeros(self.ngroups, dtype=np.int64) for f in TL_FIELDS}
        self.scalars["done_max"][:] = -1


def _count(values, bins):
    """np.bincount of int64 values known to lie in [0, bins)."""
    return np.bincount(values, minlength=bins).astype(np.uint64)


def _sum_by(index, weights, bins):
    """Per-bin integer sums (int64 throughout: no float anywhere)."""
    out = np.zeros(bins, dtype=np.int64)
    np.add.at(out, index, weights)
    return out.astype(np.uint64)


def dist_add(d, g, delays, counts, nue):
    """Adds one trial to group g of `d` (a RefDist or the package's Dist): `delays` are the timers of its successful UEs, `counts` their
    preambleTxCounter as the definition reads it, an unsigned 32-bit value (prach_internal_dist_add_ue)."""
    t = np.asarray(delays).astype(np.int64)
    p = np.asarray(counts).astype(np.int64) & 0xFFFFFFFF
    b = t // d.delay_bin_ms
    d.delay_hist[g] += _count(b[b < d.delay_bins], d.delay_bins)
    d.ptc_hist[g] += _count(np.minimum(p, PTC_BINS - 1), PTC_BINS)
    d.trials[g] += 1; d.ues[g] += int(nue); d.success[g] += t.size; d.delay_overflow[g] += int((b >= d.delay_bins).sum())
    d.delay_sum[g] += int(t.sum()); d.ptc_sum[g] += int(p.sum())
    if t.size:
        d.delay_max[g] = max(int(d.delay_max[g]), int(t.max()))


def bincount_dist(pkg, ue_arrays, bins, width, groups, ngroups):
    """np.bincount form of the distributions over int32 [nUE, 16] per-UE arrays, as the package's Dist."""
    d = pkg.Dist(ngroups, bins, width)
    for a, g in zip(ue_arrays, groups):
        ok = a[:, FLAG] == 1
        dist_add(d, g, a[ok, TIMER], a[ok, PTC], len(a))
    return d


def arrival_times(nue, sched, access_time):
    """a(i) = accessTime x the first slot s with sched[s] > i (the slot count where there is none), int64."""
    return access_time * np.searchsorted(np.asarray(sched, dtype=np.int64), np.arange(nue, dtype=np.int64), side="right")


def timeline_add(series, scalars, g, a, sched, access_time, bins, w):
    """Adds one trial (int32 [nUE, 16]) with the explicit arrival schedule `sched` to group g of (series, scalars), the two dicts of a RefTimeline
    or of the package's Timeline (include/prach.h, prach_timeline)."""
    at = arrival_times(len(a), sched, access_time)
    arrived = a[:, ACTIVE] != -1
    ok = (a[:, FLAG] == 1) & arrived
    c = a[:, TXTIME].astype(np.int64) + 6
    timer = a[:, TIMER].astype(np.int64)
    ab, db = at // w, c // w
    series["arrivals"][g] += _count(ab[arrived & (ab < bins)], bins)
    inb = ok & (ab < bins)
    series["success"][g] += _count(ab[inb], bins)
    series["sojourn_sum"][g] += _sum_by(ab[inb], (c - at)[inb], bins)
    series["timer_sum"][g] += _sum_by(ab[inb], timer[inb], bins)
    series["done"][g] += _count(db[ok & (db < bins) & (db >= 0)], bins)
    sc = scalars
    sc["trials"][g] += 1; sc["ues"][g] += len(a); sc["arrived"][g] += int(arrived.sum()); sc["success"][g] += int(ok.sum())
    sc["restarted"][g] += int((ok & (c - timer != at)).sum())
    sc["arrival_overflow"][g] += int((arrived & (ab >= bins)).sum()); sc["done_overflow"][g] += int((ok & (db >= bins)).sum())
    sc["sojourn_sum"][g] += int((c - at)[ok].sum()); sc["timer_sum"][g] += int(timer[ok].sum())
    if ok.any():
        sc["done_max"][g] = max(int(sc["done_max"][g]), int(c[ok].max()))


def same_dist(a, b, fields=DIST_FIELDS):
    """None when equal, else the first few differences as text."""
    out = []
    for name in ("delay_hist", "ptc_hist"):
        x, y = getattr(a, name), getattr(b, name)
        if x.shape != y.shape:
            return f"{name}: shapes {x.shape} {y.shape}"
        for g, k in np.argwhere(x != y)[:6]:
            out.append(f"{name}[{g}][{k}]: {int(x[g, k])} != {int(y[g, k])}")
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        for (g,) in np.argwhere(x != y)[:6]:
            out.append(f"{f}[{g}]: {int(x[g])} != {int(y[g])}")
    return "; ".join(out) or None


def same_timeline(a, b, fields=TL_FIELDS):
    out = []
    for name in TL_SERIES:
        x, y = a.series[name], b.series[name]
        if x.shape != y.shape:
            return f"{name}: shapes {x.shape} {y.shape}"
        for g, k in np.argwhere(x != y)[:6]:
            out.append(f"{name}[{g}][{k}]: {int(x[g, k])} != {int(y[g, k])}")
    for f in fields:
        x, y = a.scalars[f], b.scalars[f]
        for (g,) in np.argwhere(x != y)[:6]:
            out.append(f"{f}[{g}]: {int(x[g])} != {int(y[g])}")
    return "; ".join(out) or None


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------------

class DistJob:
    """One trial for dist_kernel: timers [nUE] (INT_MIN: not successful) and, form 0, ptc [nUE]; form 1, rec32 [nUE, 8] (word 5: count | failCount << 16)."""

    def __init__(self, timers, form, data, group):
        self.timers, self.form, self.group = np.ascontiguousarray(timers, dtype=np.int32), int(form), int(group)
        self.data = np.ascontiguousarray(data, dtype=np.int32)
        assert self.data.shape == ((len(self.timers), 8) if form else (len(self.timers),))

    @property
    def nue(self):
        return len(self.timers)

    def counts(self):
        return self.data if self.form == 0 else self.data[:, 5] & 0xFFFF

    def log(self):
        """The per-UE log a simulation kernel would have written next to this state: what the host definition reads."""
        ok = self.timers != INT_MIN
        a = np.full((self.nue, 16), PATTERN, dtype=np.int32)
        a[:, 0] = np.arange(self.nue)
        a[:, FLAG] = ok
        a[:, TIMER] = np.where(ok, self.timers, -7)
        a[:, PTC] = self.counts() if self.form == 0 else np.where(ok, self.counts(), PATTERN)
        return a


class TimelineJob:
    """One trial for timeline_kernel: logs [nUE, 16], the arrival schedule, accessTime; cfg_kw: the product config whose schedule this is (None: synthetic)."""

    def __init__(self, logs, sched, access_time, group, cfg_kw=None):
        self.logs, self.sched = np.ascontiguousarray(logs, dtype=np.int32), np.ascontiguousarray(sched, dtype=np.int32)
        self.access_time, self.group, self.cfg_kw = int(access_time), int(group), cfg_kw
        assert self.logs.shape == (len(self.logs), 16) and len(self.sched) >= 1 and (np.diff(self.sched) >= 0).all()
        assert self.sched[0] >= 0 and self.sched[-1] <= len(self.logs)

    @property
    def nue(self):
        return len(self.logs)


class Case:
    def __init__(self, kind, name, bins, width, ngroups, jobs, host):
        self.kind, self.name, self.bins, self.width, self.ngroups, self.jobs, self.host = kind, name, int(bins), int(width), int(ngroups), jobs, host
        # host: the host definition applies (dist: always; timeline: every schedule is the product's own and it accepts every log)

    def __repr__(self):
        return self.name

    def reference(self):
        if self.kind == "dist":
            d = RefDist(self.ngroups, self.bins, self.width)
            for j in self.jobs:
                ok = j.timers != INT_MIN
                dist_add(d, j.group, j.timers[ok], j.counts()[ok], j.nue)
            return d
        t = RefTimeline(self.ngroups, self.bins, self.width)
        for j in self.jobs:
            timeline_add(t.series, t.scalars, j.group, j.logs, j.sched, j.access_time, self.bins, self.width)
        return t

    def host_definition(self, pkg):
        """prach_dist_accumulate_logs / prach_timeline_accumulate_logs on logs synthesised from the same arrays."""
        groups = [j.group for j in self.jobs]
        if self.kind == "dist":
            return pkg.dist_from_logs([j.log() for j in self.jobs], self.bins, self.width, groups=groups, ngroups=self.ngroups)
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        return pkg.timeline_from_logs(cfgs, [j.logs for j in self.jobs], self.bins, self.width, groups=groups, ngroups=self.ngroups)

    def same(self, a, b):
        return same_dist(a, b) if self.kind == "dist" else same_timeline(a, b)


DIST_CASE_NAMES = ("dist_sizes_shares_patterns", "dist_bins1_width1", "dist_bins2_width3", "dist_bins16384_width1", "dist_bins16_width1048576",
                   "dist_2000_jobs_7_groups")
TIMELINE_CASE_NAMES = ("timeline_real_schedules_bins2002_width3", "timeline_real_schedules_bins65536_width1", "timeline_real_schedules_bins1_width1",
                       "timeline_one_slot_sojourn_sums", "timeline_timer_above_sojourn", "timeline_window_edges_bins65536_width1",
                       "timeline_window_edges_bins65536_width3", "timeline_window_edges_bins2002_width1", "timeline_window_edges_bins2002_width3",
                       "timeline_window_edges_bins1_width1", "timeline_schedule_ranges", "timeline_1500_jobs_5_groups")


def _sizes_all():
    return list(range(1, 10)) + [TILE - 1, TILE, TILE + 1, 3 * TILE + 1, 3 * TILE + 2, 3 * TILE + 3]


DIST_PATTERNS = ("uniform", "distinct64", "one", "edge", "high")
SHARES = ("none", "all", "sparse")


def _dist_counts(rng, n, pattern):
    i = np.arange(n)
    if pattern == "uniform" or pattern == "high":
        return rng.integers(0, 301, n)
    if pattern == "distinct64":  # lane of UE i within its tile: ((i % 1024) // 4) % 64; a wavefront votes on 64 different bins at once
        return (((i % 1024) // 4) % 64 * 3 + i // 1024 + (i % 4) * 5) % 255
    if pattern == "one":
        return np.full(n, 3)
    return rng.choice([254, 255, 256, 65535], n)


def _dist_job(rng, n, share, pattern, form, group, span):
    """span = bins x width.  Delays: uniform up to 1.2 x span, with 0, span - 1, span and INT_MAX mixed in."""
    d = rng.integers(0, min(INT_MAX, span + span // 5 + 2), n)
    pick = rng.integers(0, 20, n)
    for k, v in enumerate((0, span - 1, min(span, INT_MAX), INT_MAX)):
        d[pick == k] = v
    ok = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "sparse": rng.integers(0, 50, n) == 0}[share]
    timers = np.where(ok, d, INT_MIN)
    c = _dist_counts(rng, n, pattern)
    if form == 0:
        data = np.where(ok, c, rng.integers(1, 70000, n))  # unsuccessful UEs carry counts too: none may be counted
    else:
        hi = rng.integers(1, 65536, n) if pattern == "high" else np.zeros(n, dtype=np.int64)  # failCount, the high half of word 5
        data = rng.integers(INT_MIN, INT_MAX, (n, 8))
        w5 = c | (hi << 16)
        data[:, 5] = np.where(w5 >= 2**31, w5 - 2**32, w5)  # (the int32 it is stored as)
        data[~ok] = PATTERN
    return DistJob(timers, form, data, group)


def dist_cases():
    cases = []
    # every size x share x pattern x form around one (bins, width): the small sizes in full, the large ones with the share rotating
    rng = np.random.default_rng(101)
    bins, width = 1023, 7
    jobs = []
    for n in _sizes_all():
        k = 0
        for pattern in DIST_PATTERNS:
            for form in (0, 1):
                if pattern == "high" and form == 0:
                    continue
                for share in (SHARES if n < 10 else (SHARES[(k + n) % 3],)):
                    jobs.append(_dist_job(rng, n, share, pattern, form, len(jobs), bins * width))
                k += 1
    for form in (0, 1):  # one tile whose delays lie just below INT_MAX: the sum passes 2^32 (and 2^44)
        j = _dist_job(rng, TILE, "all", "uniform", form, len(jobs), bins * width)
        j.timers[:] = INT_MAX - rng.integers(0, 1000, TILE)
        jobs.append(j)
    cases.append(Case("dist", "dist_sizes_shares_patterns", bins, width, len(jobs), jobs, True))
    for q, (bins, width) in enumerate(((1, 1), (2, 3), (16384, 1), (16, 1 << 20))):
        rng = np.random.default_rng(110 + q)
        jobs = []
        for n in (3, 6, TILE + 1, 3 * TILE + 2):
            for pattern, form, share in (("uniform", 0, "all"), ("edge", 1, "all"), ("high", 1, "sparse"), ("distinct64", 0, "sparse")):
                jobs.append(_dist_job(rng, n, share, pattern, form, len(jobs), bins * width))
        cases.append(Case("dist", f"dist_bins{bins}_width{width}", bins, width, len(jobs), jobs, True))
    # the job table: 2000 jobs of random size into 7 groups, two of them empty
    rng = np.random.default_rng(120)
    sizes = rng.integers(1, 301, 2000)
    sizes[rng.choice(2000, 8, replace=False)] = [TILE, TILE + 1, 2 * TILE, 2 * TILE + 3, 3 * TILE, 1, TILE - 1, 2 * TILE - 2]
    jobs = [_dist_job(rng, int(n), SHARES[1 + k % 2] if k % 7 else "none", DIST_PATTERNS[k % 5] if k % 2 else DIST_PATTERNS[k % 4], k % 2,
                      (0, 1, 3, 4, 6)[int(rng.integers(0, 5))], 1023 * 7) for k, n in enumerate(sizes)]
    cases.append(Case("dist", "dist_2000_jobs_7_groups", 1023, 7, 7, jobs, True))
    return cases


def sched_from_slots(slots, nslots):
    """The schedule (UEs activated up to and including each slot) of UEs whose non-decreasing arrival slots are `slots`."""
    return np.searchsorted(np.asarray(slots, dtype=np.int64), np.arange(nslots, dtype=np.int64), side="right")


def _tl_logs(rng, at, arrived, ok, soj, timer):
    """Logs of UEs arriving at `at`: successful ones complete at at + soj with `timer`; not-arrived ones carry a set msg4Flag on every other UE and
    the pattern elsewhere, arrived unsuccessful ones the pattern in timer and txTime: none of it may be counted."""
    n = len(at)
    a = np.full((n, 16), PATTERN, dtype=np.int64)
    a[:, 0] = np.arange(n)
    a[:, ACTIVE] = np.where(arrived, np.where(ok, 0, rng.integers(1, 3, n)), -1)
    a[:, FLAG] = np.where(arrived, ok, np.arange(n) % 2)
    good = arrived & ok
    a[good, TXTIME] = (at + soj - 6)[good]
    a[good, TIMER] = np.broadcast_to(timer, (n,))[good]
    return a.astype(np.int32)


def _soj_mix(rng, n):
    soj = rng.integers(0, 3001, n)
    pick = rng.integers(0, 10, n)
    for k, v in enumerate((0, MAX_SOJOURN, MAX_SOJOURN + 1, 1 << 20)):
        soj[pick == k] = v
    return soj


def _timer_within(rng, soj):
    return (rng.random(len(soj)) * (soj + 1)).astype(np.int64)  # uniform in [0, soj]


REAL_SCHEDULES = (dict(variant=0, uniform=0, accessTime=5), dict(variant=1, uniform=0, accessTime=7), dict(variant=0, uniform=1, accessTime=1))


def _real_job(pkg, rng, n, kw, group, soj=None, timer=None, all_ok=False):
    sched = pkg.arrival_schedule(pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **kw))[0]
    at = arrival_times(n, sched, kw["accessTime"])
    arrived = np.ones(n, bool) if all_ok else rng.integers(0, 5, n) != 0
    if n > 2 * TILE and not all_ok:
        arrived[TILE:2 * TILE] = False  # a whole tile in which no UE has arrived
    ok = arrived if all_ok else arrived & (rng.integers(0, 10, n) < 7)
    soj = _soj_mix(rng, n) if soj is None else np.full(n, soj)
    timer = _timer_within(rng, soj) if timer is None else np.full(n, timer)
    return TimelineJob(_tl_logs(rng, at, arrived, ok, soj, timer), sched, kw["accessTime"], group, dict(kw))


def _window_job(rng, n, bins, width, b0, group):
    """accessTime 1.  Arrival bins b0 (the tile's anchor), b0 + 1, the last of the window, the first past it, bins - 1, bins and beyond; done bins from
    the same list, so that every pair (arrival inside / outside the window) x (done inside / outside, below / past `bins`) occurs."""
    targets = sorted({b for b in (b0, b0 + 1, b0 + WINDOW - 1, b0 + WINDOW, bins - 1, bins, bins + 5) if b >= b0})
    tb = np.array(targets)[np.sort(rng.integers(0, len(targets), n))]
    tb[0] = b0
    slots = np.sort(tb * width + rng.integers(0, width, n))  # (the first UE arrives in bin b0)
    sched = sched_from_slots(slots, int(slots[-1]) + 3)
    at = arrival_times(n, sched, 1)
    assert (at == slots).all()
    dtargets = np.array(targets + [b0 + WINDOW + 3000])
    db = dtargets[rng.integers(0, len(dtargets), n)]
    c = np.maximum(db * width + rng.integers(0, width, n), at + rng.integers(0, 4, n))
    soj = c - at
    arrived = rng.integers(0, 8, n) != 0
    arrived[0] = True
    ok = arrived & (rng.integers(0, 10, n) < 8)
    return TimelineJob(_tl_logs(rng, at, arrived, ok, soj, _timer_within(rng, soj)), sched, 1, group)


def _random_job(rng, n, group):
    access_time = int(rng.choice([1, 5, 7]))
    nslots = int(rng.integers(1, 401))
    slots = np.sort(rng.integers(0, nslots + 1, n))  # (slot nslots: no slot activates the UE)
    sched = sched_from_slots(slots, nslots)
    at = arrival_times(n, sched, access_time)
    arrived = (slots < nslots) & (rng.integers(0, 6, n) != 0)
    ok = arrived & (rng.integers(0, 10, n) < 7)
    soj = _soj_mix(rng, n)
    return TimelineJob(_tl_logs(rng, at, arrived, ok, soj, _timer_within(rng, soj)), sched, access_time, group)


def timeline_cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    cases = []
    for q, (bins, width) in enumerate(((2002, 3), (65536, 1), (1, 1))):
        rng = np.random.default_rng(201 + q)
        jobs = []
        for kw in REAL_SCHEDULES:
            for n in (1, 37, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
                jobs.append(_real_job(pkg, rng, n, kw, len(jobs) % 3 if bins == 65536 else len(jobs)))
        cases.append(Case("timeline", f"timeline_real_schedules_bins{bins}_width{width}", bins, width, 3 if bins == 65536 else len(jobs), jobs, True))

    # a full tile in ONE arrival bin, every UE successful with the same sojourn: a 32-bit sum without its guard passes 2^32
    rng = np.random.default_rng(210)
    jobs = []
    for soj in (0, MAX_SOJOURN, MAX_SOJOURN + 1, 1 << 20):
        at = np.full(TILE, 5)
        every = np.ones(TILE, bool)
        jobs.append(TimelineJob(_tl_logs(rng, at, every, every, np.full(TILE, soj), _timer_within(rng, np.full(TILE, soj))), [0, TILE, TILE], 5, len(jobs)))
    at, every = np.full(TILE, 5), np.ones(TILE, bool)  # ... and with timers far below it (UEs that started over): only the sojourn can pass the budget
    jobs.append(TimelineJob(_tl_logs(rng, at, every, every, np.full(TILE, 1 << 20), rng.integers(0, 101, TILE)), [0, TILE, TILE], 5, len(jobs)))
    cases.append(Case("timeline", "timeline_one_slot_sojourn_sums", 2002, 1, len(jobs), jobs, False))

    # the product's Beta schedule under one 10 000 ms bin: the same four sojourns, and timer = 1 << 20 above a sojourn of 100 (the definition accepts it)
    rng = np.random.default_rng(211)
    kw = REAL_SCHEDULES[0]
    jobs = [_real_job(pkg, rng, TILE, kw, k, soj=s, all_ok=True) for k, s in enumerate((0, MAX_SOJOURN, MAX_SOJOURN + 1, 1 << 20))]
    jobs.append(_real_job(pkg, rng, TILE, kw, len(jobs), soj=100, timer=1 << 20, all_ok=True))
    jobs.append(_real_job(pkg, rng, TILE + 3, kw, len(jobs), soj=MAX_SOJOURN, timer=1 << 20, all_ok=True))
    jobs.append(_real_job(pkg, rng, TILE, kw, len(jobs), soj=1 << 20, timer=5, all_ok=True))
    cases.append(Case("timeline", "timeline_timer_above_sojourn", 1, 10000, len(jobs), jobs, True))

    for q, (bins, width) in enumerate(((65536, 1), (65536, 3), (2002, 1), (2002, 3), (1, 1))):
        rng = np.random.default_rng(220 + q)
        b0 = 0 if bins == 1 else 1000
        jobs = [_window_job(rng, TILE + 5, bins, width, b0, 0), _window_job(rng, 300, bins, width, 0, 1), _window_job(rng, 2 * TILE, bins, width, b0 + 7, 2)]
        cases.append(Case("timeline", f"timeline_window_edges_bins{bins}_width{width}", bins, width, 3, jobs, False))

    # the staging edge, one slot for a whole tile, a schedule that ends below a tile, a tile that has not arrived
    rng = np.random.default_rng(230)
    jobs = []
    for per_slot in (SCHED_CAP, SCHED_CAP + 1, SCHED_CAP - 1):  # tile 1's slot range: exactly 2048 entries (staged), 2049 (searched in global memory), 2047
        slots = np.concatenate([np.full(TILE, 7), 8 + np.minimum(np.arange(TILE), per_slot)])
        sched = sched_from_slots(slots, 8 + per_slot + 3)
        for access_time in (1, 5):
            at = arrival_times(2 * TILE, sched, access_time)
            arrived = rng.integers(0, 9, 2 * TILE) != 0
            ok = arrived & (rng.integers(0, 10, 2 * TILE) < 8)
            soj = _soj_mix(rng, 2 * TILE)
            jobs.append(TimelineJob(_tl_logs(rng, at, arrived, ok, soj, _timer_within(rng, soj)), sched, access_time, len(jobs)))
    for per_slot in (SCHED_CAP, SCHED_CAP + 1):  # the same edge in a job's first tile (its range starts at slot 0), one UE per slot throughout
        slots = np.minimum(np.arange(TILE), per_slot)
        sched = sched_from_slots(slots, per_slot + 1)
        at = arrival_times(TILE, sched, 1)
        every = np.ones(TILE, bool)
        soj = _soj_mix(rng, TILE)
        jobs.append(TimelineJob(_tl_logs(rng, at, every, every, soj, _timer_within(rng, soj)), sched, 1, len(jobs)))
    n = 2 * TILE  # the schedule ends below the second tile's first UE: its UEs have no slot (a(i) = accessTime x the slot count), some logged as arrived
    slots = np.sort(rng.integers(0, 500, TILE - 100))
    sched = sched_from_slots(slots, 500)
    at = arrival_times(n, sched, 5)
    arrived = rng.integers(0, 3, n) != 0
    ok = arrived & (rng.integers(0, 10, n) < 8)
    soj = _soj_mix(rng, n)
    jobs.append(TimelineJob(_tl_logs(rng, at, arrived, ok, soj, _timer_within(rng, soj)), sched, 5, len(jobs)))
    n = 3 * TILE  # no UE of the middle tile has arrived
    slots = np.sort(rng.integers(0, 3000, n))
    sched = sched_from_slots(slots, 3000)
    at = arrival_times(n, sched, 1)
    arrived = rng.integers(0, 5, n) != 0
    arrived[TILE:2 * TILE] = False
    ok = arrived & (rng.integers(0, 10, n) < 8)
    soj = _soj_mix(rng, n)
    jobs.append(TimelineJob(_tl_logs(rng, at, arrived, ok, soj, _timer_within(rng, soj)), sched, 1, len(jobs)))
    cases.append(Case("timeline", "timeline_schedule_ranges", 65536, 1, len(jobs), jobs, False))

    # the job table: 1500 jobs into 5 groups
    rng = np.random.default_rng(240)
    sizes = rng.integers(1, 301, 1500)
    sizes[rng.choice(1500, 6, replace=False)] = [TILE, TILE + 1, 2 * TILE, 3 * TILE - 1, 1, TILE - 1]
    jobs = [_random_job(rng, int(n), int(rng.integers(0, 5))) for n in sizes]
    cases.append(Case("timeline", "timeline_1500_jobs_5_groups", 2002, 3, 5, jobs, False))
    return cases


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    kind = 0 if case.kind == "dist" else 1
    head = np.zeros(16, dtype=np.int32)
    head[:6] = [MAGIC, kind, len(case.jobs), case.bins, case.width, case.ngroups]
    if kind == 1:
        return H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group]))
    rows = np.zeros((len(case.jobs), 8), dtype=np.int32)
    rows[:, :3] = [[j.nue, j.group, j.form] for j in case.jobs]
    H.write_job_case(path, head, rows, [a for j in case.jobs for a in (j.timers, j.data.reshape(-1))])


def read_result(case, path, scheme):
    """The harness's result file as a RefDist / RefTimeline; trials and ues are the host's own count, as in the engine."""
    r = np.fromfile(path, dtype="<u8")
    ng, bins = case.ngroups, case.bins
    tile = TILE
    wgs = sum(-(-j.nue // tile) for j in case.jobs)
    assert [int(v) for v in r[:4]] == [MAGIC, 0 if case.kind == "dist" else 1, scheme, wgs], r[:4]
    r = r[4:]
    if case.kind == "dist":
        assert r.size == ng * (bins + PTC_BINS + 8)
        d = RefDist(ng, bins, case.width)
        d.delay_hist[:] = r[:ng * bins].reshape(ng, bins)
        d.ptc_hist[:] = r[ng * bins:ng * (bins + PTC_BINS)].reshape(ng, PTC_BINS)
        sc = r[ng * (bins + PTC_BINS):].reshape(ng, 8).astype(np.int64)
        d.success[:], d.delay_overflow[:], d.delay_sum[:], d.ptc_sum[:], d.delay_max[:] = sc[:, 0], sc[:, 1], sc[:, 2], sc[:, 3], sc[:, 4] - 1
        assert not sc[:, 5:].any()
        out, fields = d, (d.trials, d.ues)
    else:
        assert r.size == ng * (5 * bins + 8)
        t = RefTimeline(ng, bins, case.width)
        for q, name in enumerate(TL_SERIES):
            t.series[name][:] = r[q * ng * bins:(q + 1) * ng * bins].reshape(ng, bins)
        sc = r[5 * ng * bins:].reshape(ng, 8).astype(np.int64)
        for q, f in enumerate(("arrived", "success", "restarted", "arrival_overflow", "done_overflow", "sojourn_sum", "timer_sum")):
            t.scalars[f][:] = sc[:, q]
        t.scalars["done_max"][:] = sc[:, 7] - 1
        out, fields = t, (t.scalars["trials"], t.scalars["ues"])
    for j in case.jobs:
        fields[0][j.group] += 1
        fields[1][j.group] += j.nue
    return out


def run_harness(exe, case, case_path, scheme, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.s{scheme}.result")
    H.run(exe, [case_path, res, scheme], timeout)
    return read_result(case, res, scheme)
