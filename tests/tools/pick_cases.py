"""prach::pick_kernel away from the engine: seeded cases of per-UE state no simulation leaves behind, the kernel's raw output restated in numpy (the rows in
UE-INDEX order, the keys outside 0 .. 65 535 counted and not ranked) and the glue around tests/tools/gpu_pick_harness.hip (case file, result file, one child
process per launch).  Shared by tests/test_pick_cases_cpu.py and tests/test_gpu_pick_synthetic.py.  No GPU and no package import here."""
import ctypes
import os

import numpy as np

import harness as H
import pick_ref as P
import reduce_cases as R
import xtab_ref as X

MAX_KEY = 65535        # PK_MAX_KEY (prach_pick.hip); tests/test_pick_cases_cpu.py holds it and the rest against `gpu_pick_harness --constants`
SCHED_CAP = 12288      # PK_SCHED_CAP: a longer schedule is searched in global memory
ROW_WORDS, SCALARS = 10, 8
MAX_K = 4096
CONSTANTS = dict(PK_ROW_WORDS=ROW_WORDS, PK_SCALARS=SCALARS, PK_MAX_KEY=MAX_KEY, PK_SCHED_CAP=SCHED_CAP, PK_COARSE=1024, PK_FINE=64, PRACH_PICK_MAX_K=MAX_K,
                 PRACH_PICK_MAX_CLAUSES=4, TL_MAX_SOJOURN=60006)
THREADS = (512, 1024)  # the two workgroup shapes of the kernel
HARNESS = "gpu_pick_harness.hip"
FILL = 0x5A5A5A5A      # what the harness fills the outputs with: a row the kernel does not write
ALL = X.SERVED | X.UNSERVED | X.IDLE
SIZES = (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049)  # around a wavefront, THREADS - 1 .. THREADS + 1 and 2 THREADS + 1 of both shapes
NAMES = ("one", "arrival", "sojourn", "completion", "timer", "ptc", "failcount", "age", "state")


class Job:
    """One trial: logs [nUE, 16], the arrival schedule, accessTime, E; cfg_kw: the product config whose schedule this is (None: synthetic)."""

    def __init__(self, logs, sched, access_time, E, cfg_kw=None):
        self.logs, self.sched = np.ascontiguousarray(logs, dtype=np.int32), np.ascontiguousarray(sched, dtype=np.int32)
        self.access_time, self.E, self.cfg_kw = int(access_time), int(E), cfg_kw
        assert self.logs.shape == (len(self.logs), 16) and len(self.sched) >= 1 and (np.diff(self.sched) >= 0).all()
        assert self.sched[0] >= 0 and self.sched[-1] <= len(self.logs)

    @property
    def nue(self):
        return len(self.logs)


def raw_pick(job, where, order, key, k, who):
    """What the kernel leaves for one trial: the SCALARS words (selected, matched, stored, undefined, range_errors, threshold, ties_left_out, 0) and the
    stored rows as int32 [stored, 20] IN UE-INDEX ORDER.  A match whose key lies outside 0 .. MAX_KEY is counted in matched and in range_errors and is not
    ranked: stored, threshold and ties_left_out are those of the others."""
    a = job.logs
    match, und, keyv, sel = P.masks(a, job.sched, job.access_time, job.E, where, order, key, who)
    ranked = match & (keyv <= MAX_KEY)
    idx = np.flatnonzero(ranked)
    if order == P.LARGEST:
        idx = idx[np.lexsort((idx, -keyv[idx]))]
    elif order == P.SMALLEST:
        idx = idx[np.lexsort((idx, keyv[idx]))]
    top, rest = idx[:k], idx[k:]
    keyed = order != P.BY_INDEX and len(top) > 0
    thr = int(keyv[top[-1]]) if keyed else -1
    scalars = [int(sel.sum()), int(match.sum()), len(top), int(und.sum()), int((match & ~ranked).sum()), thr, int((keyv[rest] == thr).sum()) if keyed else 0, 0]
    top = np.sort(top)
    at = np.asarray(R.arrival_times(len(a), job.sched, job.access_time), dtype=np.int64)
    arrival = np.where(a[top, X.T.ACTIVE] == -1, -1, at[top])
    zeros = np.zeros((len(top), 2), dtype=np.int64)
    rows = np.concatenate([a[top].astype(np.int64), arrival[:, None], keyv[top][:, None], zeros], axis=1).astype(np.int32).reshape(len(top), 20)
    return scalars, rows


class Case:
    """One launch: the spec (where: clauses (field id, lo, hi); order; key field id; k; who) and the jobs, job t being trial t.  host: every schedule is the
    product's own and no key is out of range, so the host definition applies."""

    def __init__(self, name, where, order, key, k, who, jobs, host=False):
        self.name, self.where, self.order, self.key, self.k, self.who, self.jobs, self.host = name, tuple(where), int(order), int(key), int(k), int(who), jobs, host
        assert len(self.where) <= 4 and 1 <= self.k <= MAX_K and (self.order != P.BY_INDEX or self.key == 0)

    def __repr__(self):
        return self.name

    def spec(self):
        return self.where, self.order, self.key, self.k, self.who

    def reference(self):
        """(scalars int64 [njobs, SCALARS], rows int32 [njobs, k, 20]) as the harness returns them: FILL behind a trial's stored rows."""
        sc = np.zeros((len(self.jobs), SCALARS), dtype=np.int64)
        rows = np.full((len(self.jobs), self.k, 20), FILL, dtype=np.int32)
        for t, j in enumerate(self.jobs):
            s, r = raw_pick(j, *self.spec())
            sc[t] = s
            rows[t, :len(r)] = r
        return sc, rows

    def host_definition(self, pkg):
        """The host definition in the raw form: its rows sorted back into UE-index order (the 20 words of a row, FILL behind the stored ones)."""
        cfgs = [pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw) for j in self.jobs]
        pk = pkg.pick_from_logs(cfgs, [j.E for j in self.jobs], [j.logs for j in self.jobs], *self.spec())
        sc = np.zeros((len(self.jobs), SCALARS), dtype=np.int64)
        rows = np.full((len(self.jobs), self.k, 20), FILL, dtype=np.int32)
        for t in range(len(self.jobs)):
            h = pk.headers[t]
            sc[t] = [int(h[f]) for f in ("selected", "matched", "stored", "undefined", "range_errors", "threshold", "ties_left_out")] + [0]
            r = pk.rows[t, :int(h["stored"])]
            flat = np.stack([r[n] for n in r.dtype.names if n != "pad"] + [r["pad"][:, 0], r["pad"][:, 1]], axis=1).reshape(len(r), 20)
            rows[t, :len(r)] = flat[np.argsort(flat[:, 0], kind="stable")]  # (column 0 is the UE index: these jobs log idx = i)
        return sc, rows


def same(a, b):
    """None when both (scalars, rows) pairs are equal, else the first few differences as text."""
    (sa, ra), (sb, rb) = a, b
    if sa.shape != sb.shape or ra.shape != rb.shape:
        return f"shapes {sa.shape} {sb.shape} {ra.shape} {rb.shape}"
    d = [f"trial {t} scalar {w}: {int(sa[t, w])} != {int(sb[t, w])}" for t, w in np.argwhere(sa != sb)[:6]]
    d += [f"trial {t} row {r} word {w}: {int(ra[t, r, w])} != {int(rb[t, r, w])}" for t, r, w in np.argwhere(ra != rb)[:6]]
    return "; ".join(d) or None


# ---- the generators -----------------------------------------------------------------------------------------------------------------------------------

def random_job(rng, n, nslots=40, access_time=5, idle=0.15, served=0.5, timer=None, sched=None, cfg_kw=None, E=None):
    """n UEs of the three classes with every field the menu reads drawn at random (what it does not read holds reduce_cases.PATTERN): arrivals on a random
    synthetic schedule of `nslots` slots (or on `sched`), sojourns up to 60 000, timers up to 3000 (or `timer`), counts up to 300, every STATE, an E in
    front of the last arrivals (their AGE is undefined)."""
    if sched is None:
        sched = R.sched_from_slots(np.sort(rng.integers(0, nslots, n)), nslots)
    at = np.asarray(R.arrival_times(n, sched, access_time), dtype=np.int64)
    u = rng.random(n)
    is_idle, is_served = u < idle, (u >= idle) & (u < idle + served)
    a = np.full((n, 16), R.PATTERN, dtype=np.int64)
    a[:, 0] = np.arange(n)
    a[:, X.T.ACTIVE] = np.where(is_idle, -1, np.where(is_served, 0, rng.choice([1, 1, 1, 2, 2, 3], n)))
    a[:, X.T.FLAG] = np.where(is_idle, np.arange(n) % 2, is_served)
    a[:, X.T.TXTIME] = np.where(is_served, at + rng.integers(0, 60001, n) - 6, R.PATTERN)
    a[:, X.T.TIMER] = np.where(is_idle, -1, rng.integers(0, 3001, n) if timer is None else np.broadcast_to(timer, (n,)))
    a[:, X.NOWBACKOFF] = rng.integers(-3, 21, n)
    a[:, X.CONNREQ] = rng.integers(0, 61, n)
    a[:, X.PTC_COL] = rng.integers(0, 301, n)
    a[:, X.FAILCOUNT_COL] = rng.integers(0, 131, n)
    E = int(at.max() - rng.integers(0, 3) * access_time) if E is None else E
    return Job(a.astype(np.int32), sched, access_time, max(E, 0), cfg_kw)


def real_job(pkg, rng, n, kw):
    """The product's own schedule, and its E: the whole run."""
    c = pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, **kw)
    return random_job(rng, n, access_time=kw["accessTime"], sched=pkg.arrival_schedule(c)[0], cfg_kw=dict(kw), E=pkg.lib().prach_max_time(ctypes.byref(c)))


def timer_job(rng, timers):
    """Every UE arrived, with the given timers: the key of the threshold cases."""
    return random_job(rng, len(timers), idle=0.0, timer=np.asarray(timers))


def sizes_jobs(rng):
    """Every size; an idle-only trial, a trial nobody is served in and one without an unserved UE among them."""
    jobs = [random_job(rng, n) for n in SIZES]
    return jobs + [random_job(rng, 700, idle=1.0), random_job(rng, 700, idle=0.0, served=0.0), random_job(rng, 700, idle=0.3, served=0.7)]


CASE_NAMES = ("sizes_by_index", "sizes_largest_timer", "k_1", "k_matched_minus_1", "k_matched", "k_matched_plus_1", "k_max", "all_keys_equal_and_ties_across_blocks",
              "thresholds_largest", "thresholds_smallest", "one_key_65536") + tuple(f"key_{n}" for n in NAMES) + ("schedule_around_the_staging_limit", "real_schedules")
MATCHED = 100  # of every trial of the k_matched cases


def threshold_timers(rng):
    """Timers whose k-th largest / smallest, k = 50, sits at 0, at 63 and 64 (two fine bins, two coarse bins), at the edge between the coarse bins two lanes
    of the scanning wavefront own (64 511 | 64 512), and at 65 535; n = 1300 each, in random order."""
    n, k = 1300, 50
    out = []
    for lo, hi in ((0, 1), (63, 64), (64, 65), (62, 63), (64511, 64512), (64512, 64513), (65534, 65535), (0, 65535)):
        for few in (k - 3, k, k + 3):  # the k-th largest is lo, or hi with no / some ties left out; and the same for the k-th smallest
            out.append(rng.permutation(np.concatenate([np.full(few, hi), np.full(n - few, lo)])))
            out.append(rng.permutation(np.concatenate([np.full(few, lo), np.full(n - few, hi)])))
    out.append(np.full(n, 65535))
    out.append(np.zeros(n, dtype=np.int64))
    out.append(rng.integers(0, 65536, n))
    return out


def cases(pkg):
    """`pkg` gives the product's own arrival schedules (host code; no device)."""
    out = []
    arrived = X.SERVED | X.UNSERVED
    rng = np.random.default_rng(501)
    out.append(Case("sizes_by_index", [(X.STATE, 0, 3)], P.BY_INDEX, 0, 7, ALL, sizes_jobs(rng)))
    rng = np.random.default_rng(502)
    out.append(Case("sizes_largest_timer", [(X.AGE, 0, 65535)], P.LARGEST, X.TIMER, 7, ALL, sizes_jobs(rng)))
    # exactly MATCHED matches per trial (PTC 7 on MATCHED UEs, never elsewhere), failcount keys with ties
    rng = np.random.default_rng(503)
    jobs = []
    for n in (100, 513, 1025, 3000):
        j = random_job(rng, n, idle=0.0)
        j.logs[:, X.PTC_COL] = np.where(j.logs[:, X.PTC_COL] == 7, 8, j.logs[:, X.PTC_COL])
        j.logs[rng.permutation(n)[:MATCHED], X.PTC_COL] = 7
        j.logs[:, X.FAILCOUNT_COL] %= 9
        jobs.append(j)
    for name, k in (("k_1", 1), ("k_matched_minus_1", MATCHED - 1), ("k_matched", MATCHED), ("k_matched_plus_1", MATCHED + 1)):
        out.append(Case(name, [(X.PTC, 7, 7)], P.SMALLEST if k % 2 else P.LARGEST, X.FAILCOUNT, k, arrived, jobs))
    rng = np.random.default_rng(504)
    out.append(Case("k_max", [], P.LARGEST, X.PTC, MAX_K, ALL, [random_job(rng, 5000, idle=0.05), random_job(rng, 4097, idle=0.0), random_job(rng, 4096, idle=0.0),
                                                             random_job(rng, 3000), random_job(rng, 9000, idle=0.5)]))
    # k = 1100 of all-equal keys: the ties taken end at UE 1099, behind the first block of either shape; keys of a handful of values: ties on both sides of every boundary
    rng = np.random.default_rng(505)
    out.append(Case("all_keys_equal_and_ties_across_blocks", [], P.LARGEST, X.TIMER, 1100, arrived,
                    [timer_job(rng, np.full(2100, 777)), timer_job(rng, rng.integers(5, 8, 2100)), timer_job(rng, np.where(np.arange(2100) % 64 == 63, 9, 8)),
                     timer_job(rng, np.where(np.arange(2100) < 1030, 3, 4)), timer_job(rng, np.full(1100, 1)), timer_job(rng, np.full(1099, 1))]))
    rng = np.random.default_rng(506)
    tj = [timer_job(rng, t) for t in threshold_timers(rng)]
    out.append(Case("thresholds_largest", [], P.LARGEST, X.TIMER, 50, arrived, tj))
    out.append(Case("thresholds_smallest", [], P.SMALLEST, X.TIMER, 50, arrived, tj))
    # one key past the range (it would be the largest): counted, not ranked; and a trial all of whose matches are out of range
    rng = np.random.default_rng(507)
    t = rng.integers(0, 3001, 1000)
    t[500] = MAX_KEY + 1
    out.append(Case("one_key_65536", [], P.LARGEST, X.TIMER, 16, arrived, [timer_job(rng, t), timer_job(rng, np.full(70, MAX_KEY + 1)), timer_job(rng, rng.integers(0, 3001, 300))]))
    # every menu field as the key, the two fields behind it and one more as clauses
    for f, name in enumerate(NAMES):
        rng = np.random.default_rng(510 + f)
        wide = {X.ONE: (0, 0), X.ARRIVAL: (20, 150), X.SOJOURN: (1000, 50000), X.COMPLETION: (500, 40000), X.TIMER: (100, 2500), X.PTC: (10, 280), X.FAILCOUNT: (3, 120),
                X.AGE: (0, 120), X.STATE: (1, 5)}
        where = [(g, *wide[g]) for g in ((f + 1) % 9, (f + 2) % 9, (f + 5) % 9)]
        out.append(Case(f"key_{name}", where, P.LARGEST if f % 2 else P.SMALLEST, f, 33, ALL if f % 3 else arrived, [random_job(rng, n) for n in (65, 1025, 2049, 6000)]))
    rng = np.random.default_rng(520)
    jobs = [random_job(rng, 4000, nslots=ns, access_time=1) for ns in (SCHED_CAP, SCHED_CAP + 1)]  # one launch: the first schedule is staged in LDS, the second searched in global memory
    out.append(Case("schedule_around_the_staging_limit", [(X.AGE, 100, 12000)], P.SMALLEST, X.ARRIVAL, 40, ALL, jobs))
    rng = np.random.default_rng(521)
    out.append(Case("real_schedules", [(X.ARRIVAL, 0, 9000), (X.STATE, 1, 4)], P.LARGEST, X.SOJOURN, 64, ALL,
                    [real_job(pkg, rng, n, kw) for kw in R.REAL_SCHEDULES for n in (1, 65, 1025, 8193)], True))
    assert tuple(c.name for c in out) == CASE_NAMES
    return out


# ---- the harness --------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return H.build(HARNESS, out_dir)


def write_case(case, path):
    head = np.zeros(32, dtype=np.int32)
    head[:5] = [R.MAGIC, 4, len(case.jobs), case.who, len(case.where)]
    for c, cl in enumerate(case.where):
        head[5 + 3 * c:8 + 3 * c] = cl
    head[17:20] = [case.order, case.key, case.k]
    H.write_job_case(path, head, *H.log_jobs(case.jobs, lambda t, j: [t, j.E]))


def read_result(case, path, threads):
    """The harness's result file as (scalars int64 [njobs, SCALARS], rows int32 [njobs, k, 20])."""
    r = np.fromfile(path, dtype="<u8")
    n = len(case.jobs)
    assert [int(v) for v in r[:4]] == [R.MAGIC, 4, threads, n], r[:4]
    r = r[4:]
    assert r.size == n * (SCALARS + case.k * ROW_WORDS)
    return r[:n * SCALARS].view(np.int64).reshape(n, SCALARS).copy(), r[n * SCALARS:].view(np.int32).reshape(n, case.k, 20).copy()


def run_harness(exe, case, case_path, threads, out_dir, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    res = os.path.join(str(out_dir), f"{case.name}.t{threads}.result")
    H.run(exe, [case_path, res, threads], timeout)
    return read_result(case, res, threads)
