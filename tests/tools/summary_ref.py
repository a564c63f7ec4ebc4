"""numpy restatement of the per-trial summary (include/prach.h, prach_trial_summary) over per-UE arrays, shared by tests/test_summary_cpu.py,
tests/test_gpu_summary.py and the synthetic cases.  Built on timeline_ref.per_ue: arrival time, arrived, successful and completion are the timeline's.  A
level is np.sort plus the integer rank rule, in Python integers.  No GPU, no package import."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeline_ref as T  # noqa: E402

PTC = 11  # preambleTxCounter, column of the 16-field per-UE log
MAX_Q = 8
QUANTITIES = ("sojourn", "timer", "ptc")
SCALARS = ("arrived", "success", "restarted", "sojourn_sum", "timer_sum", "ptc_sum", "sojourn_max", "timer_max", "ptc_max")


def rank(n, m):
    """The rank of level m (permille) among n values: max(1, (n m + 999) // 1000)."""
    return max(1, (int(n) * int(m) + 999) // 1000)


def level(values, m):
    """The rank(n, m)-th smallest of `values`; -1 if there are none."""
    v = np.sort(np.asarray(values, dtype=np.int64))
    return int(v[rank(len(v), m) - 1]) if len(v) else -1


def trial_row(a, sched, access_time, permille):
    """The summary of one trial (int32 [nUE, 16]) as a dict: SCALARS, and q = [3][MAX_Q] levels (-1: unused, or nobody successful)."""
    at, arrived, ok, done = T.per_ue(a, sched, access_time)
    at = at.astype(np.int64)
    x = [(done - at)[ok], a[ok, T.TIMER].astype(np.int64), a[ok, PTC].astype(np.int64)]
    row = dict(arrived=int(arrived.sum()), success=int(ok.sum()), restarted=int((done - a[:, T.TIMER] != at)[ok].sum()))
    for name, v in zip(QUANTITIES, x):
        row[name + "_sum"] = int(v.sum())
        row[name + "_max"] = int(v.max()) if len(v) else -1
    row["q"] = [[level(v, permille[l]) if l < len(permille) else -1 for l in range(MAX_Q)] for v in x]
    return row


def row_as_dict(r):
    """One element of Summary.rows in the form of trial_row."""
    d = {f: int(r[f]) for f in SCALARS}
    d["q"] = np.asarray(r["q"]).tolist()
    return d


def check_rows(rows, refs, status=0):
    """Every row equals its reference (a trial_row dict), is PRACH_OK and free of range errors."""
    assert len(rows) == len(refs)
    for k, (r, ref) in enumerate(zip(rows, refs)):
        assert int(r["status"]) == status and int(r["range_errors"]) == 0, (k, int(r["status"]), int(r["range_errors"]))
        assert row_as_dict(r) == ref, (k, row_as_dict(r), ref)


def stats_ref(rows, permille, groups, ngroups):
    """prach_summary_stats in numpy: a dict (group, metric index) -> (n, mean, sd, sem, min, max); metrics in the order of the C function."""
    out = {}
    nq = len(permille)
    groups = np.asarray(groups)
    for g in range(ngroups):
        rs = rows[(groups == g) & (rows["status"] == 0)]
        has = rs[rs["success"] > 0]
        s = has["success"].astype(np.float64)
        cols = [rs["success"].astype(np.float64) / rs["nUE"].astype(np.float64), has["restarted"] / s, has["sojourn_sum"] / s, has["timer_sum"] / s, has["ptc_sum"] / s]
        cols += [has["q"][:, x, l].astype(np.float64) for x in range(3) for l in range(nq)]
        for m, v in enumerate(cols):
            n = len(v)
            sd = float(np.std(v, ddof=1)) if n > 1 else 0.0
            out[g, m] = (n, float(np.mean(v)), sd, sd / np.sqrt(n), float(v.min()), float(v.max())) if n else (0, 0.0, 0.0, 0.0, 0.0, 0.0)
    return out
