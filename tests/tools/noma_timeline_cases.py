"""prach::noma_timeline_kernel away from the engine: seeded cases of per-UE state no NOMA.c trial leaves behind — every class and STATE, sectors outside 0..5 on
arrived UEs, negative timers and transmit times on served UEs, a sojourn and a timer on and above the 32-bit tile budget, a whole tile in one (sector, bin),
tiles whose arrivals span one bin less than, exactly and one bin more than the LDS window, completions on both sides of the window's end, arrivals and
completions on both sides of the last bin, a tile nobody activated, a schedule range longer than the staged part, 1500 jobs into 3 groups — with the numpy
restatement of tests/tools/noma_timeline_ref.py as their reference, and the glue around tests/tools/gpu_noma_timeline_harness.hip (case file, result file, one
child process per launch).  Shared by tests/test_noma_timeline_cases_cpu.py and tests/test_gpu_noma_timeline_synthetic.py.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import noma_census_cases as NC
import noma_census_ref as N
import noma_timeline_ref as T
import reduce_cases as R

TILE = R.TILE
WINDOW, MAX_SOJOURN = 256, 10006  # NTL_WINDOW, NTL_MAX_SOJOURN
CONSTANTS = dict(TL_TILE=8192, TL_THREADS=256, NTL_WINDOW=WINDOW, NTL_WINDOW_MAX=1024, NTL_MAX_SOJOURN=MAX_SOJOURN, TILE_SCHED_CAP=2048, NTL_SCALARS=12)
NTL_SCALARS = 12
KIND = 13
HARNESS = "gpu_noma_timeline_harness.hip"
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
NOMA_KW = dict(variant=2, accessTime=5)  # the product's NOMA.c schedule
INT_MIN = -2 ** 31
Job = NC.Job  # a timeline job plus E


def same(a, b):
    """None when the timelines {"series", "scalars"} are equal, else the first few differences as text."""
    out = []
    if a["series"].shape != b["series"].shape:
        return f"series: shapes {a['series'].shape} {b['series'].shape}"
    for at in np.argwhere(a["series"] != b["series"])[:6]:
        out.append(f"{T.SERIES[at[0]]}{list(map(int, at[1:]))}: {int(a['series'][tuple(at)])} != {int(b['series'][tuple(at)])}")
    for f in T.SCALARS:
        x, y = a["scalars"][f], b["scalars"][f]
        for (g,) in np.argwhere(x != y)[:6]:
            out.append(f"{f}[{g}]: {int(x[g])} != {int(y[g])}")
    return "; ".join(out) or None


class Case:
    """host: every schedule is the product's own NOMA.c schedule, so the host definition applies."""

    def __init__(self, name, bins, bin_ms, ngroups, jobs, host):
        self.name, self.bins, self.bin_ms, self.ngroups, self.jobs, self.host = name, int(bins), int(bin_ms), int(ngroups), jobs, host

    def __repr__(self):
        return self.name

    def reference(self):
        return T.timeline([j.logs for j in self.jobs], [j.sched for j in self.jobs], [j.access_time for j in self.jobs], [j.E for j in self.jobs], self.bins, self.bin_ms,
                          groups=[j.group for j in self.jobs], ngroups=self.ngroups)

    def host_definition(self, pkg):
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        t = pkg.noma_timeline_from_logs(cfgs, [j.E for j in self.jobs], [j.logs for j in self.jobs], self.bins, self.bin_ms, groups=[j.group for j in self.jobs], ngroups=self.ngroups)
        return {"series": t.series.astype(np.int64), "scalars": t.scalars}


CASE_NAMES = ("real_sizes_wild_records", "real_sizes_one_bin", "budget_sojourn_and_timer", "whole_tile_one_cell", "window_spans_and_completions", "last_bin_edges",
              "tiles_nobody_activated", "long_schedule_range", "jobs_1500_groups_3")


def wild(rng, at, E):
    """noma_census_cases.wild_logs, with the sectors 6 and INT_MIN on some UEs (arrived: undefined for the timeline) next to its own -1, -2 and 7."""
    a = NC.wild_logs(rng, at, E)
    pick = rng.integers(0, 40, len(a))
    a[pick == 0, N.W_SECTOR] = 6
    a[pick == 1, N.W_SECTOR] = INT_MIN
    return a


def served(n, at, soj, timer, sector):
    """n served UEs arriving at `at`: completion at + soj, the timer and the sector given (arrays or scalars)."""
    a = np.zeros((n, 16), dtype=np.int64)
    a[:, 0] = np.arange(n)
    a[:, N.W_RA] = 1
    a[:, N.W_TXTIME] = np.asarray(at) + np.asarray(soj) - 6
    a[:, N.W_TIMER] = timer
    a[:, N.W_SECTOR] = sector
    return a.astype(np.int32)


def _real_jobs(pkg, rng, groups, sizes=SIZES):
    jobs = []
    for n in sizes:
        sched = pkg.arrival_schedule(pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **NOMA_KW))[0]
        at = R.arrival_times(n, sched, NOMA_KW["accessTime"])
        E = int(at[n // 2]) if len(jobs) % 3 == 0 else 10000
        jobs.append(Job(wild(rng, at, E), sched, NOMA_KW["accessTime"], len(jobs) % groups, E, dict(NOMA_KW)))
    return jobs


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = [Case("real_sizes_wild_records", 2002, 5, 4, _real_jobs(pkg, np.random.default_rng(1300), 4), True),
           Case("real_sizes_one_bin", 1, 10006, 2, _real_jobs(pkg, np.random.default_rng(1301), 2, (65, TILE + 1)), True)]

    # a sojourn and a timer of exactly the budget of one UE and one above, alone and together, in a tile of ordinary served UEs: all in one slot
    rng = np.random.default_rng(1310)
    n = TILE + 3
    soj, tim = rng.integers(0, 3000, n), rng.integers(0, 3000, n)
    for k, (s, t) in enumerate(((MAX_SOJOURN, 0), (MAX_SOJOURN + 1, 0), (MAX_SOJOURN, MAX_SOJOURN), (MAX_SOJOURN + 1, MAX_SOJOURN + 1), (0, MAX_SOJOURN), (0, MAX_SOJOURN + 1),
                                (2 ** 31 - 1 - 20, 5), (5, 2 ** 31 - 1))):
        soj[100 * k + 7], tim[100 * k + 7] = s, t
    a = served(n, 20, soj, tim, rng.integers(0, 6, n))
    out.append(Case("budget_sojourn_and_timer", 2100, 5, 1, [Job(a, [0, 0, 0, 0, n], 5, 0, 10000)], False))

    # a whole tile in ONE (sector, bin), every UE with the largest sojourn and timer of the budget: a 32-bit counter at TILE x NTL_MAX_SOJOURN; two tiles and one UE
    n = 2 * TILE + 1
    out.append(Case("whole_tile_one_cell", 2002, 5, 1, [Job(served(n, 0, MAX_SOJOURN, MAX_SOJOURN, 3), [n], 5, 0, 10000)], False))

    # one tile each whose arrivals span WINDOW - 1, WINDOW and WINDOW + 1 bins of 3 ms from an anchor that is not 0; completions in the window's last bin and in
    # the first behind it (and anywhere else); accessTime 1
    rng = np.random.default_rng(1320)
    jobs = []
    for g, span in enumerate((WINDOW - 1, WINDOW, WINDOW + 1)):
        n, b0, w = TILE, 11 + g, 3
        slots = np.sort(np.concatenate([[w * b0, w * (b0 + span - 1) + w - 1], rng.integers(w * b0, w * (b0 + span), n - 2)]))
        sched = R.sched_from_slots(slots, w * (b0 + span) + 40)
        at = R.arrival_times(n, sched, 1)
        assert at[0] // w == b0 and at[-1] // w == b0 + span - 1
        a = wild(rng, at, 9000)
        sv = N.classes(a) == N.SERVED
        pick = rng.integers(0, 6, n)
        for k, b in enumerate((b0 + WINDOW - 1, b0 + WINDOW)):  # completion bins: the last of the window, the first behind it
            m = sv & (pick == k) & (at <= w * b)
            a[m, N.W_TXTIME] = w * b + rng.integers(0, w, int(m.sum())) - 6
            a[m, N.W_TXTIME] = np.maximum(a[m, N.W_TXTIME], at[m] - 6)
        jobs.append(Job(a, sched, 1, g, 9000))
    out.append(Case("window_spans_and_completions", 300, 3, 3, jobs, False))

    # arrivals and completions at bins * bin_ms - 1 and bins * bin_ms: accessTime 1, 77 bins of 13 ms
    rng = np.random.default_rng(1330)
    bins, w = 77, 13
    edge = bins * w
    n = TILE + 65
    slots = np.sort(np.concatenate([[edge - 1] * 40, [edge] * 40, [edge + 1] * 10, rng.integers(edge - 300, edge + 30, n - 90)]))
    sched = R.sched_from_slots(slots, edge + 60)
    at = R.arrival_times(n, sched, 1)
    a = wild(rng, at, edge + 50)
    a[:, N.W_SECTOR] = np.where(a[:, N.W_SECTOR] == -1, -1, np.abs(a[:, N.W_SECTOR].astype(np.int64)) % 6)
    sv = N.classes(a) == N.SERVED
    pick = rng.integers(0, 4, n)
    for k, c in enumerate((edge - 1, edge)):
        m = sv & (pick == k) & (at <= c)
        a[m, N.W_TXTIME] = c - 6
    out.append(Case("last_bin_edges", bins, w, 1, [Job(a, sched, 1, 0, edge + 50)], False))

    # tiles nobody activated: of three tiles the middle one is idle by its records, and the schedule activates nobody of the last (whose records say what
    # they like: an arrival behind every slot); and a job whose schedule activates nobody at all
    rng = np.random.default_rng(1340)
    n = 3 * TILE
    slots = np.sort(rng.integers(0, 2000, 2 * TILE))
    sched = R.sched_from_slots(slots, 2000)
    assert sched[-1] == 2 * TILE
    a = wild(rng, R.arrival_times(n, sched, 5), 10000)
    a[TILE:2 * TILE, N.W_SECTOR] = -1
    a[2 * TILE:, N.W_SECTOR] = np.where(rng.integers(0, 2, TILE) == 0, -1, rng.integers(0, 6, TILE))
    b = wild(rng, np.full(70, 100), 50)
    out.append(Case("tiles_nobody_activated", 2002, 5, 2, [Job(a, sched, 5, 0, 10000), Job(b, np.zeros(20, dtype=np.int32), 5, 1, 50)], False))

    # a schedule range longer than the staged part: one tile spread over 6000 one-millisecond slots
    rng = np.random.default_rng(1350)
    n = TILE + 7
    sched = R.sched_from_slots(np.sort(rng.integers(0, 6000, n)), 6000)
    at = R.arrival_times(n, sched, 1)
    out.append(Case("long_schedule_range", 1300, 5, 2, [Job(wild(rng, at, E), sched, 1, g, E) for g, E in enumerate((6000, int(at[n // 2])))], False))

    # 1500 jobs into 3 groups
    rng = np.random.default_rng(1360)
    jobs = []
    for k in range(1500):
        n = int(rng.integers(1, 41))
        nslots = int(rng.integers(1, 60))
        sched = R.sched_from_slots(np.sort(rng.integers(0, nslots + 1, n)), nslots)
        jobs.append(Job(wild(rng, R.arrival_times(n, sched, 5), 5 * nslots), sched, 5, int(rng.integers(0, 3)), 5 * nslots))
    out.append(Case("jobs_1500_groups_3", 50, 7, 3, jobs, False))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path, window=0):
    head = np.zeros(16, dtype=np.int32)
    head[:7] = [R.MAGIC, KIND, len(case.jobs), case.bins, case.bin_ms, case.ngroups, window]
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group, j.E]))


def read_result(case, path, scheme):
    """The harness's result as {"series", "scalars"}; trials and ues are the host's own count, as in the engine."""
    r = np.fromfile(path, dtype="<u8")
    ng, bins = case.ngroups, case.bins
    wgs = sum(-(-j.nue // TILE) for j in case.jobs)
    assert [int(v) for v in r[:4]] == [R.MAGIC, KIND, scheme, wgs], r[:4]
    r = r[4:]
    assert r.size == 36 * ng * bins + ng * NTL_SCALARS
    out = T.empty(ng, bins)
    out["series"][:] = r[:36 * ng * bins].reshape(6, ng, 6, bins).astype(np.int64)
    sc = r[36 * ng * bins:].reshape(ng, NTL_SCALARS).astype(np.int64)
    for q, f in enumerate(("idle", "served", "dropped", "pending", "undefined", "restarted", "arrival_overflow", "done_overflow", "sojourn_sum", "timer_sum")):
        out["scalars"][f][:] = sc[:, q]
    out["scalars"]["done_max"][:] = sc[:, 10] - 1
    assert not sc[:, 11:].any()
    for j in case.jobs:
        out["scalars"]["trials"][j.group] += 1
        out["scalars"]["ues"][j.group] += j.nue
    return out


def run_harness(exe, case, case_path, scheme, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.s{scheme}.result")
    H.run(exe, [case_path, res, scheme], timeout)
    return read_result(case, res, scheme)
