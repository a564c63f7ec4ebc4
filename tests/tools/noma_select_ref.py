"""numpy restatement of the two per-trial selections over THE NOMA MENU (include/prach.h: prach_run_trials_noma_summary, prach_run_trials_noma_pick), written
from the prose of the header, not from the C: the summary by np.sort, the pick by a filter plus a stable sort, on top of the classes and values of
tests/tools/noma_census_ref.py.  It takes the 16 int32 words per UE, the schedule and E as data, so a test can hand it the oracle's UEs, the product's logs
or synthetic records.  Shared by tests/test_noma_select_cpu.py, tests/test_noma_select_cases_cpu.py and the GPU tests.  No GPU, no package import."""
import numpy as np

import noma_census_ref as N

MAX_VALUE = 65535  # prach_summary_max_value(): the largest value the device ranks
MAX_FIELDS, MAX_Q = 4, 8
BY_INDEX, LARGEST, SMALLEST = 0, 1, 2
ORDERS = {"index": BY_INDEX, "largest": LARGEST, "smallest": SMALLEST}
PICK_HEADER = ("status", "nUE", "selected", "matched", "stored", "undefined", "range_errors", "threshold", "ties_left_out")
SUMMARY_COUNTS = ("status", "nUE", "idle", "served", "dropped", "pending", "selected", "restarted", "range_errors")


def rank(n, m):
    """The rank of level m (permille) among n values: max(1, (n m + 999) / 1000), in integers."""
    return max(1, (int(n) * int(m) + 999) // 1000)


def summary(a, sched, access_time, E, fields, who, permille, device=False):
    """One row as a dict: the counts of SUMMARY_COUNTS, n / sum / max as lists of 4, q as int [4, 8].  device=False: THE DEFINITION (any value is ranked,
    range_errors 0).  device=True: what the device call leaves — a defined value above MAX_VALUE is a range error of its field, whose levels are -1."""
    fields = [N.field_id(f) for f in fields]
    cls = N.classes(a)
    row = {"status": 0, "nUE": len(a), "range_errors": 0}
    for name, bit in (("idle", N.IDLE), ("served", N.SERVED), ("dropped", N.DROPPED), ("pending", N.PENDING)):
        row[name] = int((cls == bit).sum())
    sel = (cls & who) != 0
    row["selected"] = int(sel.sum())
    row["restarted"] = int(((cls == N.SERVED) & (N.values(N.LOST, a, sched, access_time, E) > 0)).sum())
    row["n"], row["sum"], row["max"] = [0] * MAX_FIELDS, [0] * MAX_FIELDS, [-1] * MAX_FIELDS
    row["q"] = np.full((MAX_FIELDS, MAX_Q), -1, dtype=np.int64)
    for x, f in enumerate(fields):
        v = N.values(f, a, sched, access_time, E)
        v = np.sort(v[sel & (v >= 0)])
        row["n"][x], row["sum"][x] = len(v), int(v.sum())
        if len(v) == 0:
            continue
        row["max"][x] = int(v[-1])
        errors = int((v > MAX_VALUE).sum())
        if device and errors:
            row["range_errors"] += errors
            continue
        for l, m in enumerate(permille):
            row["q"][x, l] = v[rank(len(v), m) - 1]
    return row


def summary_same(pkg_rows, k, row):
    """Row k of a package NomaSummary against a summary() result, integer for integer."""
    r = pkg_rows[k]
    return all(int(r[f]) == row[f] for f in SUMMARY_COUNTS) and r["n"].tolist() == row["n"] and r["sum"].tolist() == row["sum"] and \
        r["max"].tolist() == row["max"] and np.array_equal(r["q"].astype(np.int64), row["q"])


def summary_describe(r):
    if isinstance(r, dict):
        return {**{f: r[f] for f in SUMMARY_COUNTS}, "n": r["n"], "sum": r["sum"], "max": r["max"], "q": r["q"].tolist()}
    return {**{f: int(r[f]) for f in SUMMARY_COUNTS}, "n": r["n"].tolist(), "sum": r["sum"].tolist(), "max": r["max"].tolist(), "q": r["q"].tolist()}


def pick(a, sched, access_time, E, where, order, key, k, who, device=False):
    """The pick of one trial: (header dict over PICK_HEADER, rows as int32 [k, 20]: the 16 logged words, a(i) or -1, the key, two zeros).  device=False: THE
    DEFINITION.  device=True: a match with a key above MAX_VALUE is a range error, which voids the trial's rows (stored 0, threshold -1, ties 0)."""
    order = ORDERS[order] if isinstance(order, str) else int(order)
    n = len(a)
    cls = N.classes(a)
    sel = (cls & who) != 0
    fails, undef = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for f, lo, hi in where:
        v = N.values(f, a, sched, access_time, E)
        undef |= v < 0
        fails |= (v >= 0) & ((v < lo) | (v > hi))
    keys = np.zeros(n, dtype=np.int64)
    if order != BY_INDEX:
        keys = N.values(key, a, sched, access_time, E)
        undef |= keys < 0
    match = sel & ~fails & ~undef
    hdr = {"status": 0, "nUE": n, "selected": int(sel.sum()), "matched": int(match.sum()), "undefined": int((sel & ~fails & undef).sum()), "range_errors": 0,
           "stored": 0, "threshold": -1, "ties_left_out": 0}
    rows = np.zeros((k, 20), dtype=np.int32)
    idx = np.flatnonzero(match)
    if device and order != BY_INDEX:
        hdr["range_errors"] = int((keys[idx] > MAX_VALUE).sum())
        if hdr["range_errors"]:
            return hdr, rows
    if order == LARGEST:
        idx = idx[np.argsort(-keys[idx], kind="stable")]
    elif order == SMALLEST:
        idx = idx[np.argsort(keys[idx], kind="stable")]
    keep = idx[:k]
    hdr["stored"] = len(keep)
    at = N.arrivals(n, sched, access_time)
    rows[:len(keep), :16] = a[keep]
    rows[:len(keep), 16] = np.where(cls[keep] == N.IDLE, -1, at[keep])
    rows[:len(keep), 17] = keys[keep]
    if order != BY_INDEX and len(keep):
        hdr["threshold"] = int(keys[keep[-1]])
        hdr["ties_left_out"] = int((keys[idx[k:]] == hdr["threshold"]).sum())
    return hdr, rows


def pick_rows_of(pkg_pick, t):
    """Trial t's rows of a package Pick as int32 [k, 20]."""
    r = pkg_pick.rows[t]
    return np.ascontiguousarray(r).view(np.int32).reshape(len(r), 20)


def pick_same(pkg_pick, t, hdr, rows):
    return all(int(pkg_pick.headers[f][t]) == hdr[f] for f in PICK_HEADER) and np.array_equal(pick_rows_of(pkg_pick, t), rows)


def pick_describe(pkg_pick, t):
    return {f: int(pkg_pick.headers[f][t]) for f in PICK_HEADER}


def stats(xs):
    """n, mean, sd, sem, min, max of a list of values: numpy's mean and sample standard deviation (everything 0 for n = 0, sd = sem = 0 for n = 1).  numpy
    adds in another order than a loop in trial order does: a comparison allows STATS_RTOL."""
    x = np.asarray(xs, dtype=np.float64)
    n = len(x)
    if n == 0:
        return (0, 0.0, 0.0, 0.0, 0.0, 0.0)
    sd = float(x.std(ddof=1)) if n > 1 else 0.0
    return (n, float(x.mean()), sd, sd / float(np.sqrt(n)) if n > 1 else 0.0, float(x.min()), float(x.max()))


# Two orders of adding n doubles differ by at most about n eps relative to the sum of the magnitudes; the groups of the tests have at most a few dozen rows of
# non-negative values (no cancellation in the mean; the deviations are squared), and the square root halves a relative error: 1e-12 is three orders above that
STATS_RTOL = 1e-12
