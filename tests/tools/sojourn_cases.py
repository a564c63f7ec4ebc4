"""prach::sojourn_kernel away from the engine: seeded cases of per-UE state no simulation leaves behind (built from the generators of reduce_cases.py), a
package-free reference shape for tests/tools/sojourn_ref.py, and the glue around tests/tools/gpu_sojourn_harness.hip (case file, result file, one child
process per launch).  Shared by tests/test_sojourn_cases_cpu.py and tests/test_gpu_sojourn_synthetic.py.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import reduce_cases as R
import sojourn_ref as S

TILE, MAX_SOJOURN = R.TILE, R.MAX_SOJOURN
WINDOW_WORDS = 28672  # SJ_WINDOW_WORDS (prach_device.h); tests/test_sojourn_cases_cpu.py holds it and the rest against `gpu_sojourn_harness --constants`
CONSTANTS = dict(TL_TILE=8192, TL_THREADS=256, TL_MAX_SOJOURN=60006, SJ_WINDOW_WORDS=WINDOW_WORDS, SJ_SCHED_CAP=2048, SJ_SCALARS=8)
FIELDS = ("trials", "ues", "arrived", "success", "restarted", "arrival_overflow", "delay_overflow", "sojourn_sum", "sojourn_max")
HARNESS = "gpu_sojourn_harness.hip"


class RefSojourn:
    """The shape of the package's Sojourn without the package."""

    def __init__(self, ngroups, arrival_bins, arrival_bin_ms, delay_bins, delay_bin_ms):
        self.ngroups, self.arrival_bins, self.arrival_bin_ms, self.delay_bins, self.delay_bin_ms = int(ngroups), int(arrival_bins), int(arrival_bin_ms), int(delay_bins), int(delay_bin_ms)
        self.hist = np.zeros((self.ngroups, self.arrival_bins, self.delay_bins), dtype=np.uint64)
        self.row_arrived = np.zeros((self.ngroups, self.arrival_bins), dtype=np.uint64)
        self.row_delay_overflow = np.zeros((self.ngroups, self.arrival_bins), dtype=np.uint64)
        self.scalars = {f: np.zeros(self.ngroups, dtype=np.int64) for f in FIELDS}
        self.scalars["sojourn_max"][:] = -1


def same(a, b):
    """None when equal, else the first few differences as text."""
    out = []
    for name in ("hist", "row_arrived", "row_delay_overflow"):
        x, y = getattr(a, name), getattr(b, name)
        if x.shape != y.shape:
            return f"{name}: shapes {x.shape} {y.shape}"
        for at in np.argwhere(x != y)[:6]:
            out.append(f"{name}{list(map(int, at))}: {int(x[tuple(at)])} != {int(y[tuple(at)])}")
    for f in FIELDS:
        x, y = a.scalars[f], b.scalars[f]
        for (g,) in np.argwhere(x != y)[:6]:
            out.append(f"{f}[{g}]: {int(x[g])} != {int(y[g])}")
    return "; ".join(out) or None


class Case:
    """spec = (rows, row_ms, delay_bins, delay_bin_ms); jobs: reduce_cases.TimelineJob; host: every schedule is the product's own."""

    def __init__(self, name, spec, ngroups, jobs, host):
        self.name, self.spec, self.ngroups, self.jobs, self.host = name, tuple(int(v) for v in spec), int(ngroups), jobs, host

    def __repr__(self):
        return self.name

    def reference(self):
        ref = RefSojourn(self.ngroups, *self.spec)
        for j in self.jobs:
            S.add_trial(ref, j.group, j.logs, j.sched, j.access_time)
        return ref

    def host_definition(self, pkg):
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        return pkg.sojourn_from_logs(cfgs, [j.logs for j in self.jobs], *self.spec, groups=[j.group for j in self.jobs], ngroups=self.ngroups)


CASE_NAMES = ("one_cell_in_window", "one_cell_behind_window", "one_cell_16384_bins", "real_schedules_21x500_2002x5", "real_schedules_4096x1_64x200",
              "real_schedules_1x1_1x1", "real_schedules_behind_last_row", "real_schedules_pooled_16384x4", "window_edges_row1", "window_edges_row3",
              "no_slot_and_idle_tiles", "jobs_1500_groups_5")


def _one_cell_jobs(rng, slot):
    """Every UE of a trial arrives in ONE slot with ONE sojourn (0, the largest a simulation reaches, one more): a whole tile in one cell.  The schedule
    is synthetic."""
    jobs = []
    for soj in (0, MAX_SOJOURN, MAX_SOJOURN + 1):
        for n in (TILE, TILE + 3):
            every = np.ones(n, bool)
            sched = [0] * slot + [n, n]
            at = np.full(n, 5 * slot)
            jobs.append(R.TimelineJob(R._tl_logs(rng, at, every, every, np.full(n, soj), R._timer_within(rng, np.full(n, soj))), sched, 5, len(jobs)))
    return jobs


def _real_jobs(pkg, rng, sizes, shared_groups=None):
    jobs = []
    for kw in R.REAL_SCHEDULES:
        for n in sizes:
            jobs.append(R._real_job(pkg, rng, n, kw, len(jobs) % shared_groups if shared_groups else len(jobs)))
    return jobs


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    # a tile in one cell: the cell inside the LDS window; behind it (16 384 bins: the window is ONE row, row 0, and the tile arrives in row 3); in a window of one row
    out.append(Case("one_cell_in_window", (4, 5, 8, 8000), 6, _one_cell_jobs(np.random.default_rng(301), 1), False))
    rng = np.random.default_rng(302)
    jobs = _one_cell_jobs(rng, 3)
    for j in jobs[:3]:  # (one UE of the first tile arrives in slot 0: it anchors the window at row 0)
        j.sched[:3] = 1
        j.logs[0, R.TXTIME] -= 15
        j.logs[0, R.TIMER] = 0
    out.append(Case("one_cell_behind_window", (8, 5, 16384, 4), 6, jobs, False))
    out.append(Case("one_cell_16384_bins", (4, 5, 16384, 4), 6, _one_cell_jobs(np.random.default_rng(303), 2), False))
    # the product's schedules, every nUE % 4 below and around a tile, a tile in which nobody arrived (n > 2 tiles), sojourns 0 .. 2^20
    # (behind_last_row: 1200 delay bins of 50 ms end exactly at the sojourn of 60 006 ms that the mix holds: the first value of the overflow)
    sizes = [1, 2, 3, 4, 5, 6, 7, 37, TILE - 1, TILE, TILE + 1, TILE + 2, TILE + 3, 2 * TILE + 1]
    for q, (name, spec, grp) in enumerate((("real_schedules_21x500_2002x5", (21, 500, 2002, 5), 4), ("real_schedules_4096x1_64x200", (4096, 1, 64, 200), 3),
                                           ("real_schedules_1x1_1x1", (1, 1, 1, 1), None), ("real_schedules_behind_last_row", (3, 100, MAX_SOJOURN // 50, 50), None),
                                           ("real_schedules_pooled_16384x4", (1, 70000, 16384, 4), 2))):
        jobs = _real_jobs(pkg, np.random.default_rng(310 + q), sizes, grp)
        out.append(Case(name, spec, grp or len(jobs), jobs, True))
    # the window's edges: with 14 delay bins it holds WINDOW_WORDS / 14 rows, the count reduce_cases._window_job aims at
    assert WINDOW_WORDS // 14 == R.WINDOW
    for name, row_ms, seed in (("window_edges_row1", 1, 320), ("window_edges_row3", 3, 321)):
        rng = np.random.default_rng(seed)
        jobs = [R._window_job(rng, TILE + 5, 4096, row_ms, 1000, 0), R._window_job(rng, 300, 4096, row_ms, 0, 1), R._window_job(rng, 2 * TILE, 4096, row_ms, 1007, 2)]
        out.append(Case(name, (4096, row_ms, 14, 430 * row_ms), 3, jobs, False))
    # UEs no slot activates (arrival = accessTime x the slot count), and a middle tile in which no UE arrived
    rng = np.random.default_rng(330)
    jobs = []
    n = 2 * TILE
    slots = np.sort(rng.integers(0, 500, TILE - 100))
    sched = R.sched_from_slots(slots, 500)
    at = R.arrival_times(n, sched, 5)
    arrived = rng.integers(0, 3, n) != 0
    ok = arrived & (rng.integers(0, 10, n) < 8)
    soj = R._soj_mix(rng, n)
    jobs.append(R.TimelineJob(R._tl_logs(rng, at, arrived, ok, soj, R._timer_within(rng, soj)), sched, 5, 0))
    n = 3 * TILE
    slots = np.sort(rng.integers(0, 3000, n))
    sched = R.sched_from_slots(slots, 3000)
    at = R.arrival_times(n, sched, 1)
    arrived = rng.integers(0, 5, n) != 0
    arrived[TILE:2 * TILE] = False
    ok = arrived & (rng.integers(0, 10, n) < 8)
    soj = R._soj_mix(rng, n)
    jobs.append(R.TimelineJob(R._tl_logs(rng, at, arrived, ok, soj, R._timer_within(rng, soj)), sched, 1, 1))
    out.append(Case("no_slot_and_idle_tiles", (25, 100, 128, 30), 2, jobs, False))  # (25 rows of 100 ms: the arrivals at 2500 ms and behind are in no row)
    # the job table: 1500 jobs into 5 groups
    rng = np.random.default_rng(340)
    sizes = rng.integers(1, 301, 1500)
    sizes[rng.choice(1500, 6, replace=False)] = [TILE, TILE + 1, 2 * TILE, 3 * TILE - 1, 1, TILE - 1]
    jobs = [R._random_job(rng, int(n), int(rng.integers(0, 5))) for n in sizes]
    out.append(Case("jobs_1500_groups_5", (64, 32, 128, 25), 5, jobs, False))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    head = np.zeros(16, dtype=np.int32)
    head[:8] = [R.MAGIC, 2, len(case.jobs), *case.spec, case.ngroups]
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group]))


def read_result(case, path, scheme):
    """The harness's result file as a RefSojourn; trials and ues are the host's own count, as in the engine."""
    r = np.fromfile(path, dtype="<u8")
    ng, (rows, _, bins, _) = case.ngroups, case.spec
    wgs = sum(-(-j.nue // TILE) for j in case.jobs)
    assert [int(v) for v in r[:4]] == [R.MAGIC, 2, scheme, wgs], r[:4]
    r = r[4:]
    assert r.size == ng * (rows * bins + 2 * rows + 8)
    out = RefSojourn(ng, *case.spec)
    out.hist[:] = r[:ng * rows * bins].reshape(ng, rows, bins)
    out.row_arrived[:] = r[ng * rows * bins:ng * rows * (bins + 1)].reshape(ng, rows)
    out.row_delay_overflow[:] = r[ng * rows * (bins + 1):ng * rows * (bins + 2)].reshape(ng, rows)
    sc = r[ng * rows * (bins + 2):].reshape(ng, 8).astype(np.int64)
    for q, f in enumerate(("arrived", "success", "restarted", "arrival_overflow", "delay_overflow", "sojourn_sum")):
        out.scalars[f][:] = sc[:, q]
    out.scalars["sojourn_max"][:] = sc[:, 6] - 1
    assert not sc[:, 7].any()
    for j in case.jobs:
        out.scalars["trials"][j.group] += 1
        out.scalars["ues"][j.group] += j.nue
    return out


def run_harness(exe, case, case_path, scheme, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.s{scheme}.result")
    H.run(exe, [case_path, res, scheme], timeout)
    return read_result(case, res, scheme)
