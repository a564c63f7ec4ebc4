"""prach::noma_census_kernel and prach::noma_columns_kernel away from the engine: seeded cases of per-UE state no NOMA.c trial leaves behind — negative
words, STATE 8, a failCount with both halves set, values at and past the last regular bin, a tile of one UE, tables one cell below, at and above the LDS
window and the per-wavefront-copy limit, schedule ranges longer than the staged part — with the numpy restatement of tests/tools/noma_census_ref.py as their
reference, and the glue around tests/tools/gpu_noma_census_harness.hip (case file, result file, one child process per launch).  Shared by
tests/test_noma_census_cases_cpu.py and tests/test_gpu_noma_census_synthetic.py.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import noma_census_ref as N
import reduce_cases as R

TILE = R.TILE
WINDOW_WORDS, COPY_CELLS = 28672, 1024  # XT_WINDOW_WORDS; NC_COPY_WORDS / the four wavefronts of a workgroup
CONSTANTS = dict(TL_TILE=8192, TL_THREADS=256, XT_WINDOW_WORDS=WINDOW_WORDS, NC_COPY_WORDS=4096, TILE_SCHED_CAP=2048, NC_SCALARS=16, NCL_SCALARS=4)
NC_SCALARS, NCL_SCALARS, GUARD, PATTERN = 16, 4, 64, 0x7FFF7FFF
HARNESS = "gpu_noma_census_harness.hip"
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
NOMA_KW = dict(variant=2, accessTime=5)  # the product's NOMA.c schedule
# the columns a case is also written as unless it names its own: the whole menu and three raw words (failCount, the sector, txTime)
COLUMN_FIELDS = tuple(range(13)) + (N.RAW + 15, N.RAW + 8, N.RAW + 3)


def same(a, b):
    """None when the censuses {"cells", "scalars"} are equal, else the first few differences as text."""
    out = []
    if a["cells"].shape != b["cells"].shape:
        return f"cells: shapes {a['cells'].shape} {b['cells'].shape}"
    for at in np.argwhere(a["cells"] != b["cells"])[:6]:
        out.append(f"cells{list(map(int, at))}: {int(a['cells'][tuple(at)])} != {int(b['cells'][tuple(at)])}")
    for f in N.SCALARS:
        x, y = a["scalars"][f], b["scalars"][f]
        for (g,) in np.argwhere(x != y)[:6]:
            out.append(f"{f}[{g}]: {int(x[g])} != {int(y[g])}")
    return "; ".join(out) or None


class Job(R.TimelineJob):
    """A timeline job plus E, the subframe the trial ended at."""

    def __init__(self, logs, sched, access_time, group, E, cfg_kw=None):
        super().__init__(logs, sched, access_time, group, cfg_kw)
        self.E = int(E)


class Case:
    """spec = (rows, cols, who), an axis (field id, width, bins); host: every schedule is the product's own NOMA.c schedule."""

    def __init__(self, name, spec, ngroups, jobs, host, columns=COLUMN_FIELDS):
        self.name, self.spec, self.ngroups, self.jobs, self.host, self.columns = name, spec, int(ngroups), jobs, host, tuple(columns)

    def __repr__(self):
        return self.name

    def reference(self):
        return N.census([j.logs for j in self.jobs], [j.sched for j in self.jobs], [j.access_time for j in self.jobs], [j.E for j in self.jobs], *self.spec,
                        groups=[j.group for j in self.jobs], ngroups=self.ngroups)

    def reference_columns(self):
        """(int32 [ncols, rows], int64 [njobs, 4] class counts idle, served, dropped, pending)"""
        data = np.concatenate([N.columns(self.columns, j.logs, j.sched, j.access_time, j.E) for j in self.jobs], axis=1)
        counts = np.array([[int((N.classes(j.logs) == b).sum()) for b in (N.IDLE, N.SERVED, N.DROPPED, N.PENDING)] for j in self.jobs], dtype=np.int64)
        return data, counts

    def cfgs(self, pkg):
        return [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]

    def host_definition(self, pkg):
        c = pkg.noma_census_from_logs(self.cfgs(pkg), [j.E for j in self.jobs], [j.logs for j in self.jobs], *self.spec, groups=[j.group for j in self.jobs], ngroups=self.ngroups)
        return {"cells": c.cells, "scalars": c.scalars}

    def host_columns(self, pkg):
        col = pkg.noma_columns_from_logs(self.cfgs(pkg), [j.E for j in self.jobs], [j.logs for j in self.jobs], list(self.columns))
        return col.data, np.stack([col.headers[f].astype(np.int64) for f in ("idle", "served", "dropped", "pending")], axis=1)


CASE_NAMES = ("real_census_who_all", "real_copies_below", "real_copies_exact", "real_copies_above", "real_window_below", "real_window_exact", "real_window_above",
              "real_one_by_one_idle", "bin_edges_and_overflows", "all_lanes_one_cell", "tiles_without_a_selected_ue", "long_schedule_and_short_runs", "raw_words_of_every_quarter")


def wild_logs(rng, at, E):
    """Records of UEs arriving at `at` with every word drawn wide: every class and STATE (8 too), negative timer, txTime, preamble and counters, a failCount
    with both halves set, with only the upper one, negative and INT_MIN, served UEs that complete before they arrive, a set RA on idle UEs, a txTime on both
    sides of E."""
    n = len(at)
    a = rng.integers(-3, 70, (n, 16)).astype(np.int64)
    a[:, 0] = np.arange(n)
    a[:, N.W_ACTIVE] = rng.choice([-1, 0, 1, 1, 1, 2, 2, 3], n)
    a[:, N.W_RA] = rng.choice([0, 0, 1, 1, 2], n)
    a[:, N.W_SECTOR] = rng.choice([-1, 0, 1, 2, 3, 4, 5, 5, 7, -2], n)
    a[:, N.W_TXTIME] = np.where(rng.integers(0, 9, n) == 0, -rng.integers(1, 40, n), np.where(rng.integers(0, 3, n) == 0, E + rng.integers(-2, 3, n), at + rng.integers(-12, 700, n)))
    a[:, N.W_TIMER] = rng.integers(-2, 700, n)
    a[:, N.W_NOWBACKOFF] = rng.integers(-2, 3, n)
    a[:, N.W_MSG3WAIT] = rng.choice([0, 0, 49, -1], n)
    a[:, N.W_PTC] = rng.integers(-1, 12, n)
    a[:, N.W_RETX] = rng.integers(-1, 11, n)
    a[:, N.W_FAIL] = rng.choice([0, 0, 0, 0, 1, 3, 0x10000, 0x30001, 0x20000, 0x7fff0000, 0x7fffffff, -1, -2 ** 31, -0x10000], n)
    return a.astype(np.int32)


def _real_jobs(pkg, rng, groups, sizes=SIZES):
    """The product's NOMA.c schedule, E inside the arrivals for every third job (the UEs behind it have no AGE) and at maxTime otherwise."""
    jobs = []
    for n in sizes:
        sched = pkg.arrival_schedule(pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **NOMA_KW))[0]
        at = R.arrival_times(n, sched, NOMA_KW["accessTime"])
        E = int(at[n // 2]) if len(jobs) % 3 == 0 else 10000
        jobs.append(Job(wild_logs(rng, at, E), sched, NOMA_KW["accessTime"], len(jobs) % groups, E, dict(NOMA_KW)))
    return jobs


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    few = (65, TILE + 1, 3000)
    real = (("real_census_who_all", ((N.ARRIVAL, 500, 20), (N.STATE, 1, 9), N.ALL), 4, SIZES),
            ("real_copies_below", ((N.ARRIVAL, 313, 32), (N.TIMER, 23, 30), N.SERVED | N.PENDING), 2, few),                # 33 x 31 = 1023 cells
            ("real_copies_exact", ((N.AGE, 313, 31), (N.SOJOURN, 23, 31), N.SERVED), 2, few),                              # 32 x 32 = 1024: the last with copies
            ("real_copies_above", ((N.COMPLETION, 250, 40), (N.LOST, 29, 24), N.SERVED | N.DROPPED), 2, few),               # 41 x 25 = 1025: one copy
            ("real_window_below", ((N.TIMER, 2, 56), (N.ARRIVAL, 20, 502), N.PENDING | N.DROPPED | N.SERVED), 2, few),      # 57 x 503 = 28 671
            ("real_window_exact", ((N.ARRIVAL, 3, 4095), (N.RETX, 1, 6), N.ALL), 2, few),                                  # 4096 x 7: exactly the window
            ("real_window_above", ((N.AGE, 200, 52), (N.TIMER, 1, 540), N.DROPPED | N.PENDING), 2, few),                   # 53 x 541: one more, global atomics
            ("real_one_by_one_idle", ((N.ONE, 1, 1), (N.STATE, 9, 1), N.IDLE), 1, SIZES))
    assert 33 * 31 == COPY_CELLS - 1 and 41 * 25 == COPY_CELLS + 1 and 57 * 503 == WINDOW_WORDS - 1 and 4096 * 7 == WINDOW_WORDS and 53 * 541 == WINDOW_WORDS + 1
    for q, (name, spec, grp, sizes) in enumerate(real):
        out.append(Case(name, spec, grp, _real_jobs(pkg, np.random.default_rng(900 + q), grp, sizes), True))

    # values on a bin's last and next first value, in the overflow bin of each axis and of both at once: MSG3FAIL in rows of 7, SECTOR in columns of 3
    rng = np.random.default_rng(920)
    jobs = []
    for n in (TILE + 1, 65):
        sched = R.sched_from_slots(np.sort(rng.integers(0, 50, n)), 50)
        a = wild_logs(rng, R.arrival_times(n, sched, 5), 250)
        a[:, N.W_FAIL] = rng.choice([0, 6, 7, 13, 14, 7 * 9 - 1, 7 * 9, 7 * 9 + 1, 0x7fff], n) << 16 | rng.choice([0, 0, 1], n)
        a[:, N.W_SECTOR] = rng.choice([0, 2, 3, 5, 6, 3 * 4 - 1, 3 * 4, 3 * 4 + 1, 2 ** 31 - 1], n)
        jobs.append(Job(a, sched, 5, len(jobs), 250))
    out.append(Case("bin_edges_and_overflows", ((N.MSG3FAIL, 7, 9), (N.SECTOR, 3, 4), N.SERVED | N.PENDING | N.DROPPED), 2, jobs, False))

    # all lanes on one cell: every UE of two tiles and ONE more (a tile of one UE) is the same stranded UE, in a table of per-wavefront copies
    n = 2 * TILE + 1
    a = np.zeros((n, 16), dtype=np.int32)
    a[:, N.W_ACTIVE], a[:, N.W_TIMER], a[:, N.W_TXTIME] = 1, 33, 4
    out.append(Case("all_lanes_one_cell", ((N.STATE, 1, 9), (N.TIMER, 10, 5), N.ALL), 1, [Job(a, [0, n], 5, 0, 10)], False))

    # tiles without a selected UE: the middle tile of three is idle throughout while the served are asked for, and the other way round in a second group
    rng = np.random.default_rng(930)
    jobs = []
    for g, idle_inside in enumerate((True, False)):
        n = 3 * TILE
        sched = R.sched_from_slots(np.sort(rng.integers(0, 2000, n)), 2000)
        a = wild_logs(rng, R.arrival_times(n, sched, 5), 10000)
        mid = np.zeros(n, bool)
        mid[TILE:2 * TILE] = True
        a[:, N.W_SECTOR] = np.where(mid == idle_inside, -1, np.abs(a[:, N.W_SECTOR]) % 6)
        a[mid, N.W_RA] = 1
        jobs.append(Job(a, sched, 5, g, 10000))
    out.append(Case("tiles_without_a_selected_ue", ((N.ARRIVAL, 1000, 9), (N.SOJOURN, 100, 6), N.SERVED), 2, jobs, False))

    # a schedule longer than the staged range: one tile spread over 6000 one-millisecond slots; E below the last arrival, equal to it, behind it, and 0
    rng = np.random.default_rng(940)
    jobs = []
    n = TILE + 7
    sched = R.sched_from_slots(np.sort(rng.integers(0, 6000, n)), 6000)
    at = R.arrival_times(n, sched, 1)
    for g, E in enumerate((int(at[-1]) - 1, int(at[-1]), 6000, 0)):
        a = wild_logs(rng, at, E)
        a[:, N.W_SECTOR] = np.abs(a[:, N.W_SECTOR]) % 6
        jobs.append(Job(a, sched, 1, g, E))
    out.append(Case("long_schedule_and_short_runs", ((N.AGE, 100, 60), (N.LOST, 50, 12), N.ALL), 4, jobs, False))

    # columns whose menu fields need neither quarter 0 nor quarter 1 (PTC reads quarter 2, ARRIVAL a(i)) next to a raw word of each of the four quarters: the
    # two optional quarters are loaded for the raw words alone.  The census beside them reads the two quarters every launch loads and nothing else
    out.append(Case("raw_words_of_every_quarter", ((N.PTC, 2, 5), (N.SECTOR, 1, 6), N.ALL), 2, _real_jobs(pkg, np.random.default_rng(950), 2, few), True,
                    columns=(N.PTC, N.RAW + 1, N.RAW + 6, N.RAW + 11, N.RAW + 12, N.ARRIVAL)))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    head = np.zeros(32, dtype=np.int32)
    head[:12] = [R.MAGIC, 9, len(case.jobs), case.spec[2], *case.spec[0], *case.spec[1], case.ngroups, len(case.columns)]
    head[12:12 + len(case.columns)] = case.columns
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group, j.E]))


def read_census(case, path, scheme):
    """The harness's census result as {"cells", "scalars"}; trials and ues are the host's own count and undefined is selected - binned, as in the engine."""
    r = np.fromfile(path, dtype="<u8")
    ng, ncell = case.ngroups, (case.spec[0][2] + 1) * (case.spec[1][2] + 1)
    wgs = sum(-(-j.nue // TILE) for j in case.jobs)
    assert [int(v) for v in r[:4]] == [R.MAGIC, 9, scheme, wgs], r[:4]
    r = r[4:]
    assert r.size == ng * (ncell + NC_SCALARS)
    out = N.empty(ng, case.spec[0], case.spec[1])
    out["cells"][:] = r[:ng * ncell].reshape(out["cells"].shape)
    sc = r[ng * ncell:].reshape(ng, NC_SCALARS).astype(np.int64)
    for q, f in enumerate(("idle", "served", "dropped", "pending", "selected", "binned", "row_sum", "col_sum")):
        out["scalars"][f][:] = sc[:, q]
    out["scalars"]["undefined"][:] = sc[:, 4] - sc[:, 5]
    out["scalars"]["row_max"][:] = sc[:, 8] - 1
    out["scalars"]["col_max"][:] = sc[:, 9] - 1
    assert not sc[:, 10:].any()
    for j in case.jobs:
        out["scalars"]["trials"][j.group] += 1
        out["scalars"]["ues"][j.group] += j.nue
    return out


def read_columns(case, path):
    """(int32 [ncols, rows], int64 [njobs, 4]) of the harness's columns result; the guard words behind the rows of every column hold the pattern."""
    raw = np.fromfile(path, dtype="<u4")
    njobs, rows, ncols = len(case.jobs), sum(j.nue for j in case.jobs), len(case.columns)
    head = raw[:8].view("<u8")
    assert [int(v) for v in head] == [R.MAGIC, 10, 0, sum(-(-j.nue // TILE) for j in case.jobs)], head
    counts = raw[8:8 + 2 * njobs * NCL_SCALARS].view("<u8").astype(np.int64).reshape(njobs, NCL_SCALARS)
    data = raw[8 + 2 * njobs * NCL_SCALARS:].view("<i4")
    assert data.size == ncols * (rows + GUARD)
    data = data.reshape(ncols, rows + GUARD)
    assert (data[:, rows:] == PATTERN).all(), "a word behind the rows of a column was written"
    return data[:, :rows], counts


def mode_args(mode):
    """The harness's own arguments for mode 0 / 1 (the census under that scheme) or "columns"."""
    return ["columns"] if mode == "columns" else ["census", mode]


def run_harness(exe, case, case_path, mode, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.{mode}.result")
    H.run(exe, [case_path, res, *mode_args(mode)], timeout)
    return read_columns(case, res) if mode == "columns" else read_census(case, res, mode)
