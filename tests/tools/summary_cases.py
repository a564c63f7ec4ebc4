"""prach::summary_kernel away from the engine: seeded cases of per-UE state no simulation leaves behind (built on the generators of reduce_cases.py), the
kernel's raw row restated in numpy, and the glue around tests/tools/gpu_summary_harness.hip (case file, result file, one child process per launch).
Shared by tests/test_summary_cases_cpu.py and tests/test_gpu_summary_synthetic.py.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import reduce_cases as R
import summary_ref as SR

MAX_VALUE = 65535      # SM_MAX_VALUE (prach_device.h); tests/test_summary_cases_cpu.py holds it and the rest against `gpu_summary_harness --constants`
SCHED_CAP = 12288      # SM_SCHED_CAP (prach_summary.hip): a longer schedule is searched in global memory
WORDS = 36             # SM_WORDS
CONSTANTS = dict(SM_WORDS=WORDS, SM_MAX_VALUE=MAX_VALUE, SM_SCHED_CAP=SCHED_CAP, SM_COARSE=1024, SM_FINE=64, PRACH_SUMMARY_MAX_Q=8, TL_MAX_SOJOURN=60006)
THREADS = (512, 1024)  # the two workgroup shapes of the kernel
HARNESS = "gpu_summary_harness.hip"
PTC = SR.PTC


def raw_row(logs, sched, access_time, levels):
    """What the kernel stores for one trial, as a list of WORDS Python integers: arrived, success, restarted, 3 range-error counts, 3 sums, 3 maxima, then
    [3][8] levels.  Counts, sums and maxima are over ALL successful UEs; a value outside 0 .. MAX_VALUE is in no histogram, so a level is the rank(n, m)-th
    smallest of the values in range, n still counting every successful UE, and -1 where that rank lies beyond them."""
    at, arrived, ok, done = SR.T.per_ue(logs, sched, access_time)
    at = at.astype(np.int64)
    x = [(done - at)[ok], logs[ok, SR.T.TIMER].astype(np.int64), logs[ok, PTC].astype(np.int64)]
    n = int(ok.sum())
    row = [int(arrived.sum()), n, int((done - logs[:, SR.T.TIMER] != at)[ok].sum())]
    row += [int(((v < 0) | (v > MAX_VALUE)).sum()) for v in x] + [int(v.sum()) for v in x] + [int(v.max()) if n else -1 for v in x]
    for v in x:
        inr = np.sort(v[(v >= 0) & (v <= MAX_VALUE)])
        for l in range(8):
            r = SR.rank(n, levels[l]) if l < len(levels) and n else 0
            row.append(int(inr[r - 1]) if 1 <= r <= len(inr) else -1)
    assert len(row) == WORDS
    return row


def logs_of(rng, at, arrived, ok, soj, timer, ptc):
    """reduce_cases._tl_logs plus the preamble count of the successful UEs (elsewhere the pattern stays: none of it may be counted)."""
    a = R._tl_logs(rng, at, arrived, ok, soj, timer)
    good = arrived & ok
    a[good, PTC] = np.broadcast_to(ptc, (len(at),))[good]
    return a


def flat_job(rng, soj, timer, ptc, arrived=None, ok=None, nslots=40, access_time=5, group=0):
    """n UEs with the given values on a random synthetic schedule of `nslots` slots (every UE is activated by some slot)."""
    n = len(soj)
    slots = np.sort(rng.integers(0, nslots, n))
    sched = R.sched_from_slots(slots, nslots)
    at = R.arrival_times(n, sched, access_time)
    every = np.ones(n, bool)
    arrived = every if arrived is None else arrived
    ok = arrived if ok is None else ok
    return R.TimelineJob(logs_of(rng, at, arrived, ok, np.asarray(soj), np.asarray(timer), np.asarray(ptc)), sched, access_time, group)


def real_job(pkg, rng, n, kw, group):
    """The product's own schedule; values a simulation could leave (sojourn up to the largest, timer within it, counts up to 200)."""
    j = R._real_job(pkg, rng, n, kw, group, soj=None)
    good = (j.logs[:, R.ACTIVE] != -1) & (j.logs[:, R.FLAG] == 1)
    at = R.arrival_times(n, j.sched, j.access_time)
    soj = rng.integers(0, R.MAX_SOJOURN + 1, n)
    j.logs[good, R.TXTIME] = (at + soj - 6)[good]
    j.logs[good, R.TIMER] = (rng.random(n) * (soj + 1)).astype(np.int64)[good]
    j.logs[good, PTC] = rng.integers(1, 201, n)[good]
    return j


class Case:
    """levels: permille; jobs: reduce_cases.TimelineJob, job k is row k; host: every schedule is the product's own and every value in range."""

    def __init__(self, name, levels, jobs, host=False):
        self.name, self.levels, self.jobs, self.host = name, tuple(int(m) for m in levels), jobs, host
        for k, j in enumerate(self.jobs):
            j.group = k

    def __repr__(self):
        return self.name

    def reference(self):
        return np.array([raw_row(j.logs, j.sched, j.access_time, self.levels) for j in self.jobs], dtype=np.int64)

    def host_definition(self, pkg):
        """The host definition's rows in the raw form (its range errors are 0 by definition)."""
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        rows = pkg.summary_from_logs(cfgs, [j.logs for j in self.jobs], self.levels).rows
        return np.array([[int(r[f]) for f in ("arrived", "success", "restarted")] + [0, 0, 0] + [int(r[f]) for f in ("sojourn_sum", "timer_sum", "ptc_sum", "sojourn_max", "timer_max", "ptc_max")] +
                         [int(v) for v in np.asarray(r["q"]).reshape(-1)] for r in rows], dtype=np.int64)


def same(a, b):
    """None when equal, else the first few differences as text."""
    if a.shape != b.shape:
        return f"shapes {a.shape} {b.shape}"
    return "; ".join(f"row {k} word {w}: {int(a[k, w])} != {int(b[k, w])}" for k, w in np.argwhere(a != b)[:8]) or None


CASE_NAMES = ("one_successful_ue", "all_on_one_value", "split_63_64", "eight_levels_eight_coarse_bins", "eight_levels_one_coarse_bin", "values_0_60005_65535",
              "one_value_65536", "sizes_real_schedules", "nobody_arrived_nobody_successful_no_slot", "orders_differ", "schedule_around_the_staging_limit",
              "jobs_1500")
EIGHT = (125, 250, 375, 500, 625, 750, 875, 1000)


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    rng = np.random.default_rng(401)
    only = np.arange(7) == 4
    out.append(Case("one_successful_ue", (1, 500, 1000), [flat_job(rng, [4321], [17], [9]), flat_job(rng, np.full(7, 100) + np.arange(7), np.arange(7), np.arange(7) + 1, ok=only)]))
    rng = np.random.default_rng(402)
    out.append(Case("all_on_one_value", (1, 500, 990, 1000), [flat_job(rng, np.full(3000, 777), np.full(3000, 777), np.full(3000, 3))]))
    rng = np.random.default_rng(403)
    v = rng.permutation(np.repeat([63, 64], 500))
    out.append(Case("split_63_64", (500, 501), [flat_job(rng, v, v[::-1].copy(), 127 - v)]))  # rank 500 is the last 63, rank 501 the first 64: two coarse bins
    rng = np.random.default_rng(404)
    v = rng.permutation(np.repeat(np.arange(8) * 64 * 17 + 100, 100) + rng.integers(0, 64, 800) - 36)
    out.append(Case("eight_levels_eight_coarse_bins", EIGHT, [flat_job(rng, v, rng.permutation(v), rng.permutation(v) // 16)]))
    rng = np.random.default_rng(405)
    out.append(Case("eight_levels_one_coarse_bin", EIGHT, [flat_job(rng, 6400 + rng.integers(0, 64, 640), 64 * 1023 + rng.integers(0, 64, 640), rng.integers(0, 64, 640))]))
    rng = np.random.default_rng(406)
    pick = np.array([0, 60005, MAX_VALUE])
    out.append(Case("values_0_60005_65535", (1, 333, 334, 666, 667, 1000), [flat_job(rng, pick[rng.integers(0, 3, 999)], pick[rng.integers(0, 3, 999)], pick[rng.integers(0, 3, 999)]),
                                                                             flat_job(rng, np.full(70, MAX_VALUE), np.zeros(70, int), np.full(70, MAX_VALUE))]))
    # one value past the range: counted, in no histogram (a bin index of 1024 would be the next quantity's bin 0), the other two quantities exact
    rng = np.random.default_rng(407)
    jobs = []
    for q in range(3):
        x = [rng.integers(0, 200, 101), rng.integers(0, 200, 101), rng.integers(1, 20, 101)]
        x[q][50] = MAX_VALUE + 1
        jobs.append(flat_job(rng, *x))
    out.append(Case("one_value_65536", (1, 500, 1000), jobs))
    rng = np.random.default_rng(408)
    jobs = [real_job(pkg, rng, n, kw, 0) for kw in R.REAL_SCHEDULES for n in (1, 63, 65, 1023, 1025, 8193)]
    out.append(Case("sizes_real_schedules", (10, 500, 950, 990, 999), jobs, True))
    rng = np.random.default_rng(409)
    n = 300
    none, every = np.zeros(n, bool), np.ones(n, bool)
    vals = (rng.integers(0, 5000, n), rng.integers(0, 5000, n), rng.integers(1, 50, n))
    jobs = [flat_job(rng, *vals, arrived=none), flat_job(rng, *vals, arrived=every, ok=none)]
    slots = np.sort(rng.integers(0, 21, n))  # slot 20 of 20: no slot activates the UE, it arrives at accessTime x 20
    sched = R.sched_from_slots(slots, 20)
    jobs.append(R.TimelineJob(logs_of(rng, R.arrival_times(n, sched, 7), every, rng.integers(0, 4, n) != 0, *vals), sched, 7, 0))
    assert (slots == 20).sum() > 3
    out.append(Case("nobody_arrived_nobody_successful_no_slot", (500, 950), jobs))
    rng = np.random.default_rng(410)
    n = 2000
    out.append(Case("orders_differ", (100, 500, 900), [flat_job(rng, np.arange(n) * 3, (n - np.arange(n)) * 7, rng.permutation(n) % 251 + 1)]))
    rng = np.random.default_rng(411)
    jobs = []
    for nslots in (SCHED_CAP, SCHED_CAP + 1):  # one launch: the first schedule is staged in LDS, the second searched in global memory
        n = 4000
        jobs.append(flat_job(rng, rng.integers(0, 3000, n), rng.integers(0, 3000, n), rng.integers(1, 30, n), arrived=rng.integers(0, 5, n) != 0, nslots=nslots, access_time=1))
    out.append(Case("schedule_around_the_staging_limit", (500, 990), jobs))
    rng = np.random.default_rng(412)
    jobs = []
    for n in rng.integers(1, 301, 1500):
        arrived = rng.integers(0, 6, n) != 0
        jobs.append(flat_job(rng, rng.integers(0, R.MAX_SOJOURN + 1, n), rng.integers(0, R.MAX_SOJOURN + 1, n), rng.integers(1, 300, n), arrived=arrived,
                             ok=arrived & (rng.integers(0, 10, n) < 7), nslots=int(rng.integers(1, 401)), access_time=int(rng.choice([1, 5, 7]))))
    out.append(Case("jobs_1500", (500, 950, 990), jobs))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    head = np.zeros(16, dtype=np.int32)
    head[:4] = [R.MAGIC, 3, len(case.jobs), len(case.levels)]
    head[4:4 + len(case.levels)] = case.levels
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group]))


def read_result(case, path, threads):
    """The harness's result file as an int64 array [njobs, WORDS]."""
    r = np.fromfile(path, dtype="<u8")
    assert [int(v) for v in r[:4]] == [R.MAGIC, 3, threads, len(case.jobs)], r[:4]
    r = r[4:]
    assert r.size == len(case.jobs) * WORDS
    return r.view(np.int64).reshape(len(case.jobs), WORDS).copy()


def run_harness(exe, case, case_path, threads, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.t{threads}.result")
    H.run(exe, [case_path, res, threads], timeout)
    return read_result(case, res, threads)
