"""numpy restatement of the outcome cross-tabulation (include/prach.h, prach_xtab) over per-UE arrays, shared by tests/test_xtab_cpu.py,
tests/test_xtab_cases_cpu.py and the GPU tests.  Built on timeline_ref.per_ue; it takes the arrival schedule and E as data, so a test can hand it the
oracle's, the product's or synthetic ones.  No GPU, no package import."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeline_ref as T  # noqa: E402

SERVED, UNSERVED, IDLE = 1, 2, 4
ONE, ARRIVAL, SOJOURN, COMPLETION, TIMER, PTC, FAILCOUNT, AGE, STATE = range(9)
NOWBACKOFF, PTC_COL, CONNREQ, FAILCOUNT_COL = 6, 11, 13, 15  # columns of the 16-field per-UE log
FIELDS = ("trials", "ues", "idle", "served", "unserved", "selected", "binned", "undefined", "row_sum", "col_sum", "row_max", "col_max")


def classes(a):
    """The class bit of every UE."""
    idle = a[:, T.ACTIVE] == -1
    served = ~idle & (a[:, T.FLAG] == 1)
    return np.where(idle, IDLE, np.where(served, SERVED, UNSERVED))


def states(a):
    cls = classes(a)
    act, nb, cr = a[:, T.ACTIVE], a[:, NOWBACKOFF], a[:, CONNREQ]
    un = np.where(act == 1, np.where(nb > 0, 2, 3), np.where(act == 2, np.where(cr < 48, 4, 5), 6))
    return np.where(cls == IDLE, 0, np.where(cls == SERVED, 1, un)).astype(np.int64)


def values(field, a, sched, access_time, E):
    """The value of `field` for every UE as int64; negative: UNDEFINED."""
    at, arrived, ok, c = T.per_ue(a, sched, access_time)
    at = np.asarray(at, dtype=np.int64)
    und = np.full(len(a), -1, dtype=np.int64)
    if field == ONE:
        return np.zeros(len(a), dtype=np.int64)
    if field == ARRIVAL:
        return np.where(arrived, at, und)
    if field == SOJOURN:
        return np.where(ok, c - at, und)
    if field == COMPLETION:
        return np.where(ok, c, und)
    if field == TIMER:
        return np.where(arrived, a[:, T.TIMER].astype(np.int64), und)
    if field == PTC:
        return np.where(arrived, a[:, PTC_COL].astype(np.int64), und)
    if field == FAILCOUNT:
        return np.where(arrived, a[:, FAILCOUNT_COL].astype(np.int64), und)
    if field == AGE:
        return np.where(arrived, np.int64(E) - at, und)
    assert field == STATE
    return states(a)


def add_trial(xt, g, a, sched, access_time, E):
    """Adds one trial (int32 [nUE, 16]) that ended at subframe E to group g of the package's Xtab `xt`, in numpy."""
    (rf, rw, rb), (cf, cw, cb) = xt.rows, xt.cols
    cls = classes(a)
    sc = xt.scalars
    sc["trials"][g] += 1
    sc["ues"][g] += len(a)
    for name, bit in (("idle", IDLE), ("served", SERVED), ("unserved", UNSERVED)):
        sc[name][g] += int((cls == bit).sum())
    sel = (cls & xt.who) != 0
    rv, cv = values(rf, a, sched, access_time, E), values(cf, a, sched, access_time, E)
    good = sel & (rv >= 0) & (cv >= 0)
    sc["selected"][g] += int(sel.sum())
    sc["binned"][g] += int(good.sum())
    sc["undefined"][g] += int((sel & ~good).sum())
    r, c = np.minimum(rv[good] // rw, rb), np.minimum(cv[good] // cw, cb)
    np.add.at(xt.cells[g], (r, c), 1)
    sc["row_sum"][g] += int(rv[good].sum())
    sc["col_sum"][g] += int(cv[good].sum())
    if good.any():
        sc["row_max"][g] = max(int(sc["row_max"][g]), int(rv[good].max()))
        sc["col_max"][g] = max(int(sc["col_max"][g]), int(cv[good].max()))


def numpy_xtab(pkg, arrays, scheds, access_times, ends, rows, cols, who, groups=None, ngroups=None):
    n = len(arrays)
    grp = list(range(n)) if groups is None else list(groups)
    xt = pkg.Xtab(ngroups if ngroups is not None else max(grp) + 1, rows, cols, who)
    for a, sched, at, E, g in zip(arrays, scheds, access_times, ends, grp):
        add_trial(xt, g, a, sched, at, E)
    return xt


def census(a):
    """UEs per STATE 0 .. 6."""
    return np.bincount(states(a), minlength=7).tolist()


def rank_quantile(vals, q, width, bins):
    """The rule of prach_xtab_quantile on raw column values (those of the overflow column included): the lower edge of the bin of the
    max(1, ceil(q * n))-th smallest, -1 if there is none or it is in the overflow."""
    v = np.sort(np.asarray(vals, dtype=np.int64))
    if len(v) == 0:
        return -1
    rank = min(max(int(np.ceil(q * len(v))), 1), len(v))
    b = int(v[rank - 1]) // width
    return b * width if b < bins else -1


def describe(xt):
    return {f: xt.scalars[f].tolist() for f in xt.scalars}
