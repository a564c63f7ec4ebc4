"""prach::columns_kernel away from the engine: the numpy restatement of the columns (int64 throughout, cast to int32 at the end), seeded cases of per-UE
state no simulation leaves behind and the glue around tests/tools/gpu_columns_harness.hip (case file, result file, one child process per launch).  Shared by
tests/test_columns_cpu.py, tests/test_columns_cases_cpu.py and the GPU tests.  No GPU and no package import here."""
import ctypes
import os

import numpy as np

import harness as H
import reduce_cases as R
import xtab_ref as X

COL_MAX, COL_RAW, NFIELDS = 16, 16, 9
TILE, THREADS, TILE_SCHED_CAP = 8192, 256, 2048  # TL_TILE, TL_THREADS, TILE_SCHED_CAP; tests/test_columns_cases_cpu.py holds them against `gpu_columns_harness --constants`
CL_SCALARS = 4
CONSTANTS = dict(TL_TILE=TILE, TL_THREADS=THREADS, TILE_SCHED_CAP=TILE_SCHED_CAP, CL_SCALARS=CL_SCALARS, CL_SUMS=3, PRACH_COL_MAX=COL_MAX, PRACH_COL_RAW=COL_RAW,
                 PRACH_XTAB_NFIELDS=NFIELDS)
HARNESS = "gpu_columns_harness.hip"
FILL = 0x5A5A5A5A  # what the harness fills the arena with: a word the kernel does not write
NAMES = ("one", "arrival", "sojourn", "completion", "timer", "ptc", "failcount", "age", "state")
MENU = tuple(range(NFIELDS))
RAW = tuple(range(COL_RAW, COL_RAW + 16))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def numpy_columns(a, sched, access_time, E, fields):
    """The columns of one trial (int32 [nUE, 16] log words) as int32 [ncols, nUE]: a menu field from xtab_ref.values in int64, -1 where negative (UNDEFINED),
    the low 32 bits otherwise; a raw field (COL_RAW + w) is log word w."""
    out = np.empty((len(fields), len(a)), dtype=np.int32)
    for c, f in enumerate(fields):
        if f >= COL_RAW:
            out[c] = a[:, f - COL_RAW]
        else:
            v = X.values(f, a, sched, access_time, E)
            out[c] = np.where(v < 0, -1, v).astype(np.int64).astype(np.int32)
    return out


def numpy_classes(a):
    """(idle, served, unserved) of one trial."""
    cls = X.classes(a)
    return [int((cls == b).sum()) for b in (X.IDLE, X.SERVED, X.UNSERVED)]


class Job:
    """One trial: logs [nUE, 16], the arrival schedule, accessTime, E; lead: guard words in front of its segment of every column (the offsets of the trials
    behind it move with it); cfg_kw: the product config whose schedule this is (None: synthetic)."""

    def __init__(self, logs, sched, access_time, E, lead=1, cfg_kw=None):
        self.logs, self.sched = np.ascontiguousarray(logs, dtype=np.int32), np.ascontiguousarray(sched, dtype=np.int32)
        self.access_time, self.E, self.lead, self.cfg_kw = int(access_time), int(E), int(lead), cfg_kw
        assert self.logs.shape == (len(self.logs), 16) and len(self.sched) >= 1 and (np.diff(self.sched) >= 0).all() and self.lead >= 1
        assert self.sched[0] >= 0 and self.sched[-1] <= len(self.logs)

    @property
    def nue(self):
        return len(self.logs)


class Case:
    """One launch: the fields of the columns and the jobs, job t being trial t.  host: every schedule is the product's own, so the host definition applies."""

    def __init__(self, name, fields, jobs, tail=3, host=False):
        self.name, self.fields, self.jobs, self.tail, self.host = name, tuple(int(f) for f in fields), jobs, int(tail), host
        assert 1 <= len(self.fields) <= COL_MAX

    def __repr__(self):
        return self.name

    def offsets(self):
        off, rows = [], 0
        for j in self.jobs:
            rows += j.lead
            off.append(rows)
            rows += j.nue
        return off, rows + self.tail

    def reference(self, columns=numpy_columns):
        """(offsets, scalars int64 [njobs, CL_SCALARS], data int32 [ncols, rows_cap]) as the harness returns them: FILL in every guard word."""
        off, cap = self.offsets()
        sc = np.zeros((len(self.jobs), CL_SCALARS), dtype=np.int64)
        data = np.full((len(self.fields), cap), FILL, dtype=np.int32)
        for t, j in enumerate(self.jobs):
            sc[t, :3] = numpy_classes(j.logs)
            data[:, off[t]:off[t] + j.nue] = columns(j.logs, j.sched, j.access_time, j.E, self.fields)
        return np.asarray(off, dtype=np.int64), sc, data

    def host_definition(self, pkg):
        """The host definition (prach_columns_from_logs) in the harness's form."""
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        col = pkg.columns_from_logs(cfgs, [j.E for j in self.jobs], [j.logs for j in self.jobs], self.fields)
        it = iter(range(len(self.jobs)))
        off, sc, data = self.reference(lambda a, *_: col.trial(next(it)))
        sc[:, :3] = np.stack([col.headers[n] for n in ("idle", "served", "unserved")], axis=1)
        return off, sc, data


def same(a, b):
    """None when both (offsets, scalars, data) triples are equal, else the first few differences as text."""
    (oa, sa, da), (ob, sb, db) = a, b
    if oa.shape != ob.shape or sa.shape != sb.shape or da.shape != db.shape:
        return f"shapes {oa.shape} {ob.shape} {sa.shape} {sb.shape} {da.shape} {db.shape}"
    d = [f"offset of trial {t}: {int(oa[t])} != {int(ob[t])}" for t, in np.argwhere(oa != ob)[:6]]
    d += [f"trial {t} scalar {w}: {int(sa[t, w])} != {int(sb[t, w])}" for t, w in np.argwhere(sa != sb)[:6]]
    d += [f"column {c} row {r}: {int(da[c, r])} != {int(db[c, r])}" for c, r in np.argwhere(da != db)[:6]]
    return "; ".join(d) or None


# ---- the generators -----------------------------------------------------------------------------------------------------------------------------------

def random_job(rng, n, nslots=40, access_time=5, idle=0.15, served=0.5, sched=None, cfg_kw=None, E=None, lead=1):
    """n UEs of the three classes with EVERY word of the record drawn at random around the values the menu asks about: nowBackoff around 0, connectionRequest
    around 48, active in -1 .. 3, msg4Flag 0 .. 2; completions before the arrival among the served; an E in front of the last arrivals (their AGE is
    undefined); INT_MIN and INT_MAX sprinkled over every word but active and msg4Flag."""
    if sched is None:
        sched = R.sched_from_slots(np.sort(rng.integers(0, nslots, n)), nslots)
    at = np.asarray(R.arrival_times(n, sched, access_time), dtype=np.int64)
    u = rng.random(n)
    is_idle, is_served = u < idle, (u >= idle) & (u < idle + served)
    a = rng.integers(-5, 70000, (n, 16))
    a[:, 0] = np.arange(n)
    a[:, X.T.ACTIVE] = np.where(is_idle, -1, np.where(is_served, rng.integers(0, 3, n), rng.choice([0, 1, 1, 1, 2, 2, 3], n)))
    a[:, X.T.FLAG] = np.where(is_idle, rng.integers(0, 3, n), np.where(is_served, 1, rng.choice([0, 0, 2], n)))
    a[:, X.T.TXTIME] = np.where(rng.random(n) < 0.1, at - 6 - rng.integers(1, 50, n), at + rng.integers(0, 60001, n) - 6)  # (a tenth: c(i) < a(i))
    a[:, X.T.TIMER] = np.where(is_idle, -1, rng.integers(-2, 3001, n))
    a[:, X.NOWBACKOFF] = rng.integers(-1, 3, n)
    a[:, X.CONNREQ] = rng.integers(46, 50, n)
    a[:, X.PTC_COL] = rng.integers(0, 301, n)
    a[:, X.FAILCOUNT_COL] = rng.integers(0, 131, n)
    for w in range(1, 16):
        if w not in (X.T.ACTIVE, X.T.FLAG):
            hit = rng.random(n) < 0.02
            a[hit, w] = rng.choice([INT_MIN, INT_MAX], int(hit.sum()))
    E = int(at.max() - rng.integers(1, 4) * access_time) if E is None else E
    return Job(a.astype(np.int32), sched, access_time, max(E, 0), lead, cfg_kw)


def real_job(pkg, rng, n, kw, lead=1):
    """The product's own schedule, and its E: the whole run."""
    c = pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **kw)
    return random_job(rng, n, access_time=kw["accessTime"], sched=pkg.arrival_schedule(c)[0], cfg_kw=dict(kw), E=pkg.lib().prach_max_time(ctypes.byref(c)), lead=lead)


def threshold_job(lead=1):
    """Every combination of the words the classes and STATE are decided on, at both sides of every threshold: active -1 .. 3, msg4Flag 0 .. 2, nowBackoff
    -1 .. 1, connectionRequest 47 / 48."""
    rows = [(act, m4, nb, cr) for act in (-1, 0, 1, 2, 3) for m4 in (0, 1, 2) for nb in (-1, 0, 1) for cr in (47, 48)]
    n = len(rows)
    a = np.full((n, 16), 7, dtype=np.int64)
    a[:, 0] = np.arange(n)
    a[:, [X.T.ACTIVE, X.T.FLAG, X.NOWBACKOFF, X.CONNREQ]] = rows
    a[:, X.T.TXTIME] = 100 + np.arange(n)
    return Job(a.astype(np.int32), R.sched_from_slots(np.arange(n) // 8, 20), 5, 60, lead)


SIZES = (1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193)
LEADS = (3, 1, 4, 7, 5, 6, 1, 2, 6, 6)  # the offsets of the trials take every residue mod 4 rows; odd offsets behind the trials of 8191 and 8192 UEs
CASE_NAMES = ("sizes_all_menu", "sizes_all_raw", "one_column_arrival", "one_column_raw_timer", "sixteen_columns_mixed", "repeated_fields", "thresholds",
              "no_arrival_no_optional_quarters", "schedules_around_the_staging_limit", "very_different_sizes", "real_schedules", "raw_words_of_every_quarter")


def sizes_jobs(rng):
    return [random_job(rng, n, lead=l) for n, l in zip(SIZES, LEADS)]


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    rng = np.random.default_rng(601)
    out.append(Case("sizes_all_menu", MENU, sizes_jobs(rng)))
    rng = np.random.default_rng(602)
    out.append(Case("sizes_all_raw", RAW, sizes_jobs(rng)))
    rng = np.random.default_rng(603)
    out.append(Case("one_column_arrival", [X.ARRIVAL], sizes_jobs(rng), tail=1))
    rng = np.random.default_rng(604)
    out.append(Case("one_column_raw_timer", [COL_RAW + X.T.TIMER], sizes_jobs(rng), tail=2))
    rng = np.random.default_rng(605)
    mixed = [X.STATE, COL_RAW + 6, X.AGE, COL_RAW + 11, X.SOJOURN, COL_RAW + 0, X.PTC, COL_RAW + 15, X.ONE, COL_RAW + 4, X.TIMER, COL_RAW + 9, X.COMPLETION, COL_RAW + 13, X.FAILCOUNT, X.ARRIVAL]
    out.append(Case("sixteen_columns_mixed", mixed, sizes_jobs(rng)))
    rng = np.random.default_rng(606)
    out.append(Case("repeated_fields", [X.SOJOURN, X.SOJOURN, COL_RAW + 3, X.STATE, COL_RAW + 3, X.SOJOURN], [random_job(rng, n, lead=l) for n, l in ((700, 3), (65, 2), (9000, 1))]))
    out.append(Case("thresholds", list(MENU) + [COL_RAW + w for w in (X.T.ACTIVE, X.T.FLAG, X.NOWBACKOFF, X.CONNREQ)], [threshold_job(1), threshold_job(2), threshold_job(3)]))
    # neither a(i) nor words 4-11: the schedule is not searched and the two middle quarters of a record are not read
    rng = np.random.default_rng(607)
    out.append(Case("no_arrival_no_optional_quarters", [X.TIMER, X.FAILCOUNT, X.COMPLETION, X.ONE, COL_RAW + 1, COL_RAW + 14], [random_job(rng, n, lead=l) for n, l in ((3000, 1), (8193, 3))]))
    # a tile whose slot range has 2047 / 2048 / 2049 entries: staged in LDS up to TILE_SCHED_CAP, searched in global memory past it (shi - slo = the slots the
    # tile spans); one UE per slot from slot 0 on, accessTime 1
    rng = np.random.default_rng(608)
    jobs = []
    for span, lead in ((TILE_SCHED_CAP - 1, 1), (TILE_SCHED_CAP, 2), (TILE_SCHED_CAP + 1, 3)):
        n = span + 1
        jobs.append(random_job(rng, n, access_time=1, sched=R.sched_from_slots(np.arange(n), n + 5), lead=lead))
    out.append(Case("schedules_around_the_staging_limit", [X.ARRIVAL, X.AGE, X.SOJOURN], jobs))
    rng = np.random.default_rng(609)
    out.append(Case("very_different_sizes", [X.STATE, X.AGE, COL_RAW + 11], [random_job(rng, n, lead=l) for n, l in ((1, 1), (40000, 2), (3, 3), (8192, 1), (2, 1), (17000, 6), (1, 1))]))
    rng = np.random.default_rng(610)
    out.append(Case("real_schedules", list(MENU) + [COL_RAW + 3], [real_job(pkg, rng, n, kw, lead=1 + q) for kw in R.REAL_SCHEDULES for q, n in enumerate((1, 65, 1025, 8193))], host=True))
    # menu fields that need neither optional quarter (TIMER; AGE needs a(i)) next to a raw word of each of the four quarters: quarters 1 and 2 are loaded for the raw words alone
    rng = np.random.default_rng(611)
    out.append(Case("raw_words_of_every_quarter", [X.TIMER, COL_RAW + 2, COL_RAW + 5, COL_RAW + 10, COL_RAW + 14, X.AGE], [random_job(rng, n, lead=l) for n, l in ((700, 2), (8193, 1))]))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    head = np.zeros(32, dtype=np.int32)
    head[:4] = [R.MAGIC, 5, len(case.jobs), len(case.fields)]
    head[4:4 + len(case.fields)] = case.fields
    head[20] = case.tail
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda t, j: [t, j.E, j.lead]))


def read_result(case, path):
    """The harness's result file as (offsets int64 [njobs], scalars int64 [njobs, CL_SCALARS], data int32 [ncols, rows_cap])."""
    r = np.fromfile(path, dtype="<i4")
    n, nc = len(case.jobs), len(case.fields)
    cap = case.offsets()[1]
    assert [int(v) for v in r[:5]] == [R.MAGIC, 5, n, nc, cap], r[:5]
    r = r[8:]
    assert r.size == 2 * n + 2 * n * CL_SCALARS + nc * cap
    off = r[:2 * n].copy().view(np.int64)
    sc = r[2 * n:2 * n + 2 * n * CL_SCALARS].copy().view(np.int64).reshape(n, CL_SCALARS)
    return off, sc, r[2 * n + 2 * n * CL_SCALARS:].reshape(nc, cap).copy()


def run_harness(exe, case, case_path, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.result")
    H.run(exe, [case_path, res], timeout)
    return read_result(case, res)
