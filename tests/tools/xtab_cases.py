"""prach::xtab_kernel away from the engine: seeded cases of per-UE state no simulation leaves behind, a package-free reference shape for
tests/tools/xtab_ref.py, and the glue around tests/tools/gpu_xtab_harness.hip (case file, result file, one child process per launch).  Shared by
tests/test_xtab_cases_cpu.py and tests/test_gpu_xtab_synthetic.py.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import reduce_cases as R
import xtab_ref as X

TILE = R.TILE
WINDOW_WORDS = 28672  # XT_WINDOW_WORDS (prach_device.h); tests/test_xtab_cases_cpu.py holds it and the rest against `gpu_xtab_harness --constants`
CONSTANTS = dict(TL_TILE=8192, TL_THREADS=256, XT_WINDOW_WORDS=WINDOW_WORDS, XT_COPY_WORDS=4096, XT_SCHED_CAP=2048, XT_SCALARS=16)
SCALARS = 16
FIELDS = X.FIELDS
HARNESS = "gpu_xtab_harness.hip"
ALL = X.SERVED | X.UNSERVED | X.IDLE
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)  # nUE 1, 63 / 64 / 65, 8191 / 8192 / 8193 and 16 385


class RefXtab:
    """The shape of the package's Xtab without the package."""

    def __init__(self, ngroups, rows, cols, who):
        self.ngroups, self.rows, self.cols, self.who = int(ngroups), tuple(int(v) for v in rows), tuple(int(v) for v in cols), int(who)
        self.cells = np.zeros((self.ngroups, self.rows[2] + 1, self.cols[2] + 1), dtype=np.uint64)
        self.scalars = {f: np.zeros(self.ngroups, dtype=np.int64) for f in FIELDS}
        self.scalars["row_max"][:] = -1
        self.scalars["col_max"][:] = -1


def same(a, b):
    """None when equal, else the first few differences as text."""
    out = []
    if a.cells.shape != b.cells.shape:
        return f"cells: shapes {a.cells.shape} {b.cells.shape}"
    for at in np.argwhere(a.cells != b.cells)[:6]:
        out.append(f"cells{list(map(int, at))}: {int(a.cells[tuple(at)])} != {int(b.cells[tuple(at)])}")
    for f in FIELDS:
        x, y = a.scalars[f], b.scalars[f]
        for (g,) in np.argwhere(x != y)[:6]:
            out.append(f"{f}[{g}]: {int(x[g])} != {int(y[g])}")
    return "; ".join(out) or None


class Job(R.TimelineJob):
    """A timeline job plus E, the subframe the trial ended at."""

    def __init__(self, logs, sched, access_time, group, E, cfg_kw=None):
        super().__init__(logs, sched, access_time, group, cfg_kw)
        self.E = int(E)


class Case:
    """spec = (rows, cols, who), an axis (field id, width, bins); host: every schedule is the product's own."""

    def __init__(self, name, spec, ngroups, jobs, host):
        self.name, self.spec, self.ngroups, self.jobs, self.host = name, spec, int(ngroups), jobs, host

    def __repr__(self):
        return self.name

    def reference(self):
        ref = RefXtab(self.ngroups, *self.spec)
        for j in self.jobs:
            X.add_trial(ref, j.group, j.logs, j.sched, j.access_time, j.E)
        return ref

    def host_definition(self, pkg):
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        return pkg.xtab_from_logs(cfgs, [j.E for j in self.jobs], [j.logs for j in self.jobs], *self.spec, groups=[j.group for j in self.jobs], ngroups=self.ngroups)


CASE_NAMES = ("real_census_who_all", "real_ages_unserved", "real_window_exact_served", "real_window_plus_one_arrived", "real_one_by_one_idle", "real_ptc_failcount_idle_served",
              "real_sojourn_completion_idle_unserved", "bin_edges_and_overflows", "all_lanes_one_cell", "tiles_without_a_selected_ue", "long_schedule_and_short_runs")


def wild_logs(rng, at):
    """Logs of UEs arriving at `at` with every word drawn wide: every class and STATE (6 too), negative timer, txTime and failCount, served UEs that
    complete before they arrive, a set msg4Flag on idle UEs."""
    n = len(at)
    a = rng.integers(-3, 70, (n, 16)).astype(np.int64)
    a[:, 0] = np.arange(n)
    a[:, R.ACTIVE] = rng.choice([-1, 0, 1, 1, 2, 2, 3], n)
    a[:, R.FLAG] = rng.integers(0, 3, n)
    a[:, R.TXTIME] = np.where(rng.integers(0, 9, n) == 0, -rng.integers(1, 40, n), at + rng.integers(-12, 700, n))
    a[:, R.TIMER] = rng.integers(-2, 700, n)
    a[:, X.NOWBACKOFF] = rng.integers(-2, 3, n)
    a[:, X.CONNREQ] = rng.integers(44, 52, n)
    a[:, X.PTC_COL] = rng.integers(-1, 12, n)
    a[:, X.FAILCOUNT_COL] = rng.integers(-1, 130, n)
    return a.astype(np.int32)


def _real_jobs(pkg, rng, groups):
    """The product's schedules (Beta arrivals at 5 and 7 ms slots, Uniform arrivals at 1 ms slots), every size of SIZES, E inside the arrivals for every
    third job (the UEs behind it have no AGE) and at maxTime otherwise."""
    jobs = []
    for kw in R.REAL_SCHEDULES:
        for n in SIZES:
            cfg = pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **kw)
            sched = pkg.arrival_schedule(cfg)[0]
            at = R.arrival_times(n, sched, kw["accessTime"])
            E = int(at[n // 2]) if len(jobs) % 3 == 0 else pkg.lib().prach_max_time(cfg)
            jobs.append(Job(wild_logs(rng, at), sched, kw["accessTime"], len(jobs) % groups, E, dict(kw)))
    return jobs


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    real = (("real_census_who_all", ((X.ARRIVAL, 500, 20), (X.STATE, 1, 7), ALL), 4),
            ("real_ages_unserved", ((X.ARRIVAL, 500, 20), (X.AGE, 5, 2002), X.UNSERVED), 3),
            ("real_window_exact_served", ((X.ARRIVAL, 3, 4095), (X.TIMER, 60, 6), X.SERVED), 2),             # 4096 x 7 cells: exactly the window
            ("real_window_plus_one_arrived", ((X.AGE, 200, 52), (X.TIMER, 1, 540), X.SERVED | X.UNSERVED), 2),  # 53 x 541 cells: one more
            ("real_one_by_one_idle", ((X.ONE, 1, 1), (X.STATE, 7, 1), X.IDLE), 1),
            ("real_ptc_failcount_idle_served", ((X.PTC, 2, 5), (X.FAILCOUNT, 13, 9), X.IDLE | X.SERVED), 5),
            ("real_sojourn_completion_idle_unserved", ((X.SOJOURN, 7, 90), (X.COMPLETION, 333, 31), X.IDLE | X.UNSERVED), 2))  # (nobody selected has either value)
    assert 4096 * 7 == WINDOW_WORDS and 53 * 541 == WINDOW_WORDS + 1
    for q, (name, spec, grp) in enumerate(real):
        out.append(Case(name, spec, grp, _real_jobs(pkg, np.random.default_rng(400 + q), grp), True))

    # values on a bin's last and next first value, in the overflow bin of each axis and of both at once: timer in rows of 7, preambleTxCounter in columns of 3
    rng = np.random.default_rng(420)
    jobs = []
    for n in (TILE + 1, 65):
        sched = R.sched_from_slots(np.sort(rng.integers(0, 50, n)), 50)
        a = wild_logs(rng, R.arrival_times(n, sched, 5))
        a[:, R.ACTIVE] = rng.choice([0, 1, 2], n)
        a[:, R.TIMER] = rng.choice([0, 6, 7, 13, 14, 7 * 9 - 1, 7 * 9, 7 * 9 + 1, 2 ** 31 - 1], n)
        a[:, X.PTC_COL] = rng.choice([0, 2, 3, 5, 6, 3 * 4 - 1, 3 * 4, 3 * 4 + 1, 2 ** 31 - 1], n)
        jobs.append(Job(a, sched, 5, len(jobs), 250))
    out.append(Case("bin_edges_and_overflows", ((X.TIMER, 7, 9), (X.PTC, 3, 4), X.SERVED | X.UNSERVED), 2, jobs, False))

    # all lanes on one cell: every UE of two tiles is the same UE, once in a table of per-wavefront copies
    n = 2 * TILE
    a = np.zeros((n, 16), dtype=np.int32)
    a[:, R.ACTIVE], a[:, X.NOWBACKOFF], a[:, R.TIMER] = 1, 4, 33
    out.append(Case("all_lanes_one_cell", ((X.STATE, 1, 7), (X.TIMER, 10, 5), ALL), 1, [Job(a, [0, n], 5, 0, 10)], False))

    # tiles without a selected UE: the middle tile of three is idle throughout while the served are asked for, and the other way round in a second group
    rng = np.random.default_rng(430)
    jobs = []
    for g, inner in enumerate((-1, 0)):
        n = 3 * TILE
        sched = R.sched_from_slots(np.sort(rng.integers(0, 2000, n)), 2000)
        a = wild_logs(rng, R.arrival_times(n, sched, 5))
        a[:, R.ACTIVE] = np.where(a[:, R.ACTIVE] == -1, 1, a[:, R.ACTIVE]) if inner == -1 else -1
        a[TILE:2 * TILE, R.ACTIVE] = inner
        a[TILE:2 * TILE, R.FLAG] = 1
        jobs.append(Job(a, sched, 5, g, 10000))
    out.append(Case("tiles_without_a_selected_ue", ((X.ARRIVAL, 1000, 9), (X.SOJOURN, 100, 6), X.SERVED), 2, jobs, False))

    # a schedule longer than the staged range: one tile spread over 6000 one-millisecond slots; E below the last arrival, equal to it, and behind it
    rng = np.random.default_rng(440)
    jobs = []
    n = TILE + 7
    sched = R.sched_from_slots(np.sort(rng.integers(0, 6000, n)), 6000)
    at = R.arrival_times(n, sched, 1)
    for g, E in enumerate((int(at[-1]) - 1, int(at[-1]), 6000, 0)):
        a = wild_logs(rng, at)
        a[:, R.ACTIVE] = rng.choice([1, 2], n)
        jobs.append(Job(a, sched, 1, g, E))
    out.append(Case("long_schedule_and_short_runs", ((X.AGE, 100, 60), (X.ARRIVAL, 1000, 5), X.UNSERVED | X.SERVED), 4, jobs, False))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    head = np.zeros(16, dtype=np.int32)
    head[:11] = [R.MAGIC, 3, len(case.jobs), case.spec[2], *case.spec[0], *case.spec[1], case.ngroups]
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group, j.E]))


def read_result(case, path, scheme):
    """The harness's result file as a RefXtab; trials and ues are the host's own count and undefined is selected - binned, as in the engine."""
    r = np.fromfile(path, dtype="<u8")
    ng, ncell = case.ngroups, (case.spec[0][2] + 1) * (case.spec[1][2] + 1)
    wgs = sum(-(-j.nue // TILE) for j in case.jobs)
    assert [int(v) for v in r[:4]] == [R.MAGIC, 3, scheme, wgs], r[:4]
    r = r[4:]
    assert r.size == ng * (ncell + SCALARS)
    out = RefXtab(ng, *case.spec)
    out.cells[:] = r[:ng * ncell].reshape(out.cells.shape)
    sc = r[ng * ncell:].reshape(ng, SCALARS).astype(np.int64)
    for q, f in enumerate(("idle", "served", "unserved", "selected", "binned", "row_sum", "col_sum")):
        out.scalars[f][:] = sc[:, q]
    out.scalars["undefined"][:] = sc[:, 3] - sc[:, 4]
    out.scalars["row_max"][:] = sc[:, 7] - 1
    out.scalars["col_max"][:] = sc[:, 8] - 1
    assert not sc[:, 9:].any()
    for j in case.jobs:
        out.scalars["trials"][j.group] += 1
        out.scalars["ues"][j.group] += j.nue
    return out


def run_harness(exe, case, case_path, scheme, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.s{scheme}.result")
    H.run(exe, [case_path, res, scheme], timeout)
    return read_result(case, res, scheme)
