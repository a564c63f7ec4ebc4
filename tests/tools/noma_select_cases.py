"""prach::noma_summary_kernel and prach::noma_pick_kernel away from the engine: seeded cases of per-UE state no NOMA.c trial leaves behind — the smallest
shapes at which these kernels can go wrong: trials of one UE and around a wavefront and a block of THREADS, schedules at and one past the staged part, E
below, at and behind the last arrival and 0, every class and STATE (8 too), negative words, values on the fine / coarse edge, at the end of the ranked range
and one past it, ranks that are exact and rounded up, targets sharing a fine histogram, ties on the threshold across a wavefront and a block edge — with the
numpy restatement of tests/tools/noma_select_ref.py as their reference, and the glue around tests/tools/gpu_noma_select_harness.hip (case file, result file,
one child process per launch).  A CASE is one launch: a kind, a spec and its trials (jobs); every case runs under both THREADS instantiations.  Shared by
tests/test_noma_select_cases_cpu.py and tests/test_gpu_noma_select_synthetic.py.  No GPU and no package import here."""
import os

import numpy as np

import harness as H
import noma_census_cases as NC
import noma_census_ref as N
import noma_select_ref as S
import reduce_cases as R

CONSTANTS = dict(NS_SCHED_CAP=12288, NS_COARSE=1024, NS_FINE=64, NS_MAX_KEY=65535, NSM_WORDS=54, PK_ROW_WORDS=10, PK_SCALARS=8, NSM_LDS_WORDS=6284, NS_LDS_WORDS=1168)
SCHED_CAP, NSM_WORDS, GUARD, PATTERN = 12288, 54, 64, 0x7FFF7FFF
THREADS = (512, 1024)
HARNESS = "gpu_noma_select_harness.hip"
SIZES = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049)
ARRIVED = N.SERVED | N.PENDING | N.DROPPED
Job = NC.Job


class Case:
    """kind "summary": spec = (fields, who, permille); kind "pick": spec = (where, order, key, k, who), fields as ids.  host: every schedule is the product's
    own NOMA.c schedule, so the host definitions apply (no case with host=True holds a value above the ranked range)."""

    def __init__(self, name, spec, jobs, host):
        self.kind, self.name, self.spec, self.jobs, self.host = name.split("_")[0], name, spec, jobs, host
        assert self.kind in ("summary", "pick")

    def __repr__(self):
        return self.name

    def reference(self):
        """What the device call leaves, trial by trial: summary rows (dicts), or (header, rows) pairs of the pick in the DEFINED order."""
        fn = S.summary if self.kind == "summary" else S.pick
        return [fn(j.logs, j.sched, j.access_time, j.E, *self.spec, device=True) for j in self.jobs]

    def cfgs(self, pkg):
        return [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]

    def host_definition(self, pkg):
        args = (self.cfgs(pkg), [j.E for j in self.jobs], [j.logs for j in self.jobs], *self.spec)
        return pkg.noma_summary_from_logs(*args) if self.kind == "summary" else pkg.noma_pick_from_logs(*args)


CASE_NAMES = ("summary_sizes_eight_levels", "summary_values_and_ranks", "summary_undefined_field_and_one", "summary_schedules_and_ends", "pick_index_k1_sizes",
              "pick_index_k4096_four_clauses", "pick_largest_ties", "pick_smallest_ties", "pick_largest_age_schedules_and_ends", "pick_index_idle_rows")


def _real_jobs(pkg, rng, sizes=SIZES):
    jobs = NC._real_jobs(pkg, rng, 1, sizes)
    for g, j in enumerate(jobs):
        j.group = g
    return jobs


def _arrived(n, timers, served=False):
    """n arrived UEs (sector 0, active 1: pending, STATE 5 with E behind txTime 4) that all arrive in slot 0, with the given logged timers."""
    a = np.zeros((n, 16), dtype=np.int32)
    a[:, 0] = np.arange(n)
    a[:, N.W_ACTIVE], a[:, N.W_TXTIME] = 1, 4
    a[:, N.W_TIMER] = timers
    if served:
        a[:, N.W_RA] = 1
    return a


def _value_job(values, group, ptc=None):
    """One trial whose UEs all arrive at 0 and whose TIMER values are `values`; PTC is the UE index modulo 7 unless given."""
    n = len(values)
    a = _arrived(n, values)
    a[:, N.W_PTC] = np.arange(n) % 7 if ptc is None else ptc
    return Job(a, [n], 5, group, 10)


def _schedule_jobs(rng):
    """Schedules of SCHED_CAP and SCHED_CAP + 1 one-millisecond slots (the latter is not staged); E below the last arrival, equal to it, behind it, and 0."""
    jobs = []
    n = 1500
    for nslots in (SCHED_CAP, SCHED_CAP + 1):
        sched = R.sched_from_slots(np.sort(rng.integers(0, nslots, n)), nslots)
        at = R.arrival_times(n, sched, 1)
        for E in (int(at[-1]) - 1, int(at[-1]), nslots, 0):
            a = NC.wild_logs(rng, at, E)
            a[:, N.W_SECTOR] = np.where(rng.integers(0, 8, n) == 0, -1, np.abs(a[:, N.W_SECTOR]) % 6)
            jobs.append(Job(a, sched, 1, len(jobs), E))
    return jobs


def _tie_jobs(mirror):
    """Trials of 3000 arrived UEs for k = 64 by TIMER: 20 keys above the threshold BEHIND the ties, 44 + L ties on it whose run starts at `start` — so the 44
    that are taken straddle a wavefront edge (63 / 64), the block edge of 512 threads (511 / 512) or that of 1024 (1023 / 1024) — L = 0, 3, 1000 left out,
    and keys below everywhere else; then trials with 63, 64 and 65 matches in all (no threshold pass below 65), and keys 0 and 65 535 only.  mirror: the keys
    are 65 535 - key, for SMALLEST."""
    jobs = []
    for start in (50, 490, 1000):
        for left_out in (0, 3, 1000):
            key = np.full(3000, 100, dtype=np.int64)
            key[start:start + 44 + left_out] = 500
            key[2500:2520] = 900
            jobs.append(_value_job(65535 - key if mirror else key, len(jobs)))
    for matches in (63, 64, 65):
        key = np.full(2049, -1, dtype=np.int64)  # a negative timer is undefined: no match
        key[np.linspace(0, 2048, matches).astype(int)] = np.arange(matches) % 5 * 64  # ties on every key, on the fine / coarse edge
        jobs.append(_value_job(np.where(key < 0, -1, 65535 - key if mirror else key), len(jobs)))
    key = np.where(np.arange(700) % 3 == 0, 65535, 0)
    jobs.append(_value_job(key, len(jobs)))
    # one key one past the ranked range among good ones, and a trial of nothing but that: range errors, the trial's rows are void
    key = np.full(600, 7, dtype=np.int64)
    key[333] = 65536
    jobs.append(_value_job(key, len(jobs)))
    jobs.append(_value_job(np.full(70, 65536, dtype=np.int64), len(jobs)))
    return jobs


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    # every size with every word drawn wide, the product's schedules: four fields, one of them twice, eight levels
    out.append(Case("summary_sizes_eight_levels", ((N.TIMER, N.SOJOURN, N.TIMER, N.STATE), N.ALL, (1, 1000, 500, 250, 750, 900, 990, 999)),
                    _real_jobs(pkg, np.random.default_rng(1000)), True))

    # values and ranks by TIMER (PTC next to it stays intact where TIMER has a range error)
    rng = np.random.default_rng(1010)
    jobs = [_value_job(v, g) for g, v in enumerate((
        [0, 63, 64, 65535], [0], [65535], [63, 64] * 40, rng.permutation(np.r_[np.arange(0, 600), [63, 64, 65535, 0]]),
        np.r_[rng.integers(0, 65536, 999), [65536]],           # one 65 536: a range error of TIMER, its levels are -1
        np.full(777, 4242),                                     # all values equal
        rng.integers(128, 192, 1500),                           # eight levels in ONE coarse bin: one fine histogram for all of them
        rng.permutation(1000) * 60, rng.permutation(1001) * 60,  # n of 1000 and 1001: rank 500 exact, 501 rounded up
        rng.integers(0, 65536, 2049)))]
    out.append(Case("summary_values_and_ranks", ((N.TIMER, N.PTC), ARRIVED, (1, 1000, 500, 250, 750, 900, 990, 999)), jobs, False))

    # SOJOURN is undefined for every selected UE (who = pending): n = 0, levels -1; ONE: two levels in coarse bin 0
    out.append(Case("summary_undefined_field_and_one", ((N.SOJOURN, N.ONE), N.PENDING, (500, 990)), _real_jobs(pkg, np.random.default_rng(1020)), True))
    out.append(Case("summary_schedules_and_ends", ((N.AGE, N.LOST, N.PREAMBLE, N.ARRIVAL), N.ALL, (500,)), _schedule_jobs(np.random.default_rng(1030)), False))

    out.append(Case("pick_index_k1_sizes", ((), S.BY_INDEX, N.ONE, 1, N.ALL), _real_jobs(pkg, np.random.default_rng(1040)), True))

    # k = 4096 with four clauses, one of them (SOJOURN) undefined for everybody but the served: a clause that fails next to it does not count in `undefined`.
    # Wide records in every size, then 5000 UEs of which exactly 0, 4095, 4096 and 4097 match
    where = ((N.SOJOURN, 0, 100000), (N.TIMER, 10, 600), (N.STATE, 1, 8), (N.SECTOR, 0, 5))
    jobs = _real_jobs(pkg, np.random.default_rng(1050))
    for matches in (0, 4095, 4096, 4097):
        a = _arrived(5000, 20, served=True)
        a[np.random.default_rng(1051 + matches).permutation(5000)[matches:], N.W_TIMER] = 601  # fails TIMER
        a[::9, N.W_SECTOR] = np.where(a[::9, N.W_TIMER] == 601, -1, 0)                        # idle among the failing ones: not selected under who = arrived
        jobs.append(Job(a, [5000], 5, len(jobs), 10))
    out.append(Case("pick_index_k4096_four_clauses", (where, S.BY_INDEX, N.ONE, 4096, ARRIVED), jobs, False))

    out.append(Case("pick_largest_ties", ((), S.LARGEST, N.TIMER, 64, N.ALL), _tie_jobs(False), False))
    out.append(Case("pick_smallest_ties", ((), S.SMALLEST, N.TIMER, 64, N.ALL), _tie_jobs(True), False))
    out.append(Case("pick_largest_age_schedules_and_ends", (((N.STATE, 2, 8),), S.LARGEST, N.AGE, 4096, N.ALL), _schedule_jobs(np.random.default_rng(1060)), False))
    # idle UEs among the stored rows (wild records: one sector in ten is -1), three blocks of either shape: their arrival is -1
    out.append(Case("pick_index_idle_rows", ((), S.BY_INDEX, N.ONE, 300, N.ALL), _real_jobs(pkg, np.random.default_rng(1070), (1025, 2049)), True))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def spec_words(case):
    """The 15 / 17 words of a case's spec, as prach_noma_summary_spec / prach_pick_spec lay them out (without the reserved words)."""
    if case.kind == "summary":
        fields, who, permille = case.spec
        return [who, len(fields), *(list(fields) + [0] * 4)[:4], len(permille), *(list(permille) + [0] * 8)[:8]]
    where, order, key, k, who = case.spec
    flat = [w for cl in where for w in cl]
    return [who, len(where), *(flat + [0] * 12)[:12], order, key, k]


def write_case(case, path):
    head = np.zeros(32, dtype=np.int32)
    head[:3] = [R.MAGIC, 11 if case.kind == "summary" else 12, len(case.jobs)]
    words = spec_words(case)
    head[4:4 + len(words)] = words
    assert all(j.group == k for k, j in enumerate(case.jobs))
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda k, j: [j.group, j.E]))


def read_summary(case, path, threads):
    """The harness's rows as dicts like S.summary's, unpacked the way the engine does it: a field with range errors has levels -1."""
    r = np.fromfile(path, dtype="<i8")
    nf, nq = len(case.spec[0]), len(case.spec[2])
    assert [int(v) for v in r[:4]] == [R.MAGIC, 11, threads, len(case.jobs)], r[:4]
    r = r[4:].reshape(len(case.jobs), NSM_WORDS)
    out = []
    for j, q in zip(case.jobs, r):
        row = {"status": 0, "nUE": j.nue, "idle": int(q[0]), "served": int(q[1]), "dropped": int(q[2]), "pending": int(q[3]), "selected": int(q[4]), "restarted": int(q[5]),
               "range_errors": int(q[6:6 + nf].sum()), "n": [0] * 4, "sum": [0] * 4, "max": [-1] * 4, "q": np.full((4, 8), -1, dtype=np.int64)}
        for x in range(nf):
            row["n"][x], row["sum"][x], row["max"][x] = int(q[10 + x]), int(q[14 + x]), int(q[18 + x])
            if not q[6 + x]:
                row["q"][x, :nq] = q[22 + 8 * x:22 + 8 * x + nq]
        row["raw_levels"] = q[22:].reshape(4, 8).copy()  # as the kernel wrote them
        row["unused"] = [int(v) for x in range(4) for v in (q[6 + x], q[10 + x], q[14 + x]) if x >= nf]
        out.append(row)
    return out


def summary_same(got, ref):
    """None when a harness row equals a reference row, else the differences as text."""
    out = [f"{f}: {got[f]} != {ref[f]}" for f in S.SUMMARY_COUNTS + ("n", "sum", "max") if got[f] != ref[f]]
    if not np.array_equal(got["q"], ref["q"]):
        out.append(f"q: {got['q'].tolist()} != {ref['q'].tolist()}")
    return "; ".join(out) or None


def read_pick(case, path, threads):
    """The harness's picks as (header, rows int32 [k, 20]) pairs like S.pick's, unpacked the way the engine does it: range errors void a trial's rows, the rows
    of a trial are sorted into the defined order by a stable sort on the key.  Asserts what only the raw buffer shows: the stored rows are in ascending UE
    index, the rows behind them and the guard words behind the last trial were never written."""
    raw = np.fromfile(path, dtype="<i4")
    k, order, njobs = case.spec[3], case.spec[1], len(case.jobs)
    assert [int(v) for v in raw[:8].view("<i8")] == [R.MAGIC, 12, threads, njobs], raw[:8]
    sc = raw[8:8 + 16 * njobs].view("<i8").reshape(njobs, 8)
    rows = raw[8 + 16 * njobs:]
    assert rows.size == njobs * k * 20 + GUARD
    assert (rows[njobs * k * 20:] == PATTERN).all(), "a word behind the last trial's rows was written"
    rows = rows[:njobs * k * 20].reshape(njobs, k, 20)
    out = []
    for j, q, r in zip(case.jobs, sc, rows):
        stored = int(q[2])
        assert 0 <= stored <= k and q[7] == 0
        assert (r[stored:] == PATTERN).all(), "a row behind `stored` was written"
        assert (np.diff(r[:stored, 0]) > 0).all() and not r[:stored, 18:].any(), "the kernel's rows are in ascending UE index, their last two words zero"
        hdr = {"status": 0, "nUE": j.nue, "selected": int(q[0]), "matched": int(q[1]), "undefined": int(q[3]), "range_errors": int(q[4]), "stored": stored,
               "threshold": int(q[5]), "ties_left_out": int(q[6])}
        final = np.zeros((k, 20), dtype=np.int32)
        if hdr["range_errors"]:
            hdr.update(stored=0, threshold=-1, ties_left_out=0)
        else:
            keep = r[:stored]
            if order == S.LARGEST:
                keep = keep[np.argsort(-keep[:, 17].astype(np.int64), kind="stable")]
            elif order == S.SMALLEST:
                keep = keep[np.argsort(keep[:, 17], kind="stable")]
            final[:stored] = keep
        out.append((hdr, final))
    return out


def pick_same(got, ref):
    (gh, gr), (rh, rr) = got, ref
    out = [f"{f}: {gh[f]} != {rh[f]}" for f in S.PICK_HEADER if gh[f] != rh[f]]
    if not np.array_equal(gr, rr):
        bad = np.argwhere((gr != rr).any(axis=1))[:4].ravel().tolist()
        out.append(f"rows {bad} differ: {gr[bad[0]].tolist()} != {rr[bad[0]].tolist()}")
    return "; ".join(out) or None


def host_rows(case, host):
    """A host definition's output in the form of reference()."""
    if case.kind == "summary":
        return [{**{f: int(r[f]) for f in S.SUMMARY_COUNTS}, "n": r["n"].tolist(), "sum": r["sum"].tolist(), "max": r["max"].tolist(), "q": r["q"].astype(np.int64)}
                for r in host.rows]
    return [({f: int(host.headers[f][t]) for f in S.PICK_HEADER}, S.pick_rows_of(host, t)) for t in range(len(case.jobs))]


def same(case, got, ref):
    fn = summary_same if case.kind == "summary" else pick_same
    bad = [f"trial {t} (nUE {case.jobs[t].nue}): {fn(g, r)}" for t, (g, r) in enumerate(zip(got, ref)) if fn(g, r)]
    return "; ".join(bad[:3]) or None


def run_harness(exe, case, case_path, threads, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.{threads}.result")
    H.run(exe, [case_path, res, threads], timeout)
    return read_summary(case, res, threads) if case.kind == "summary" else read_pick(case, res, threads)
