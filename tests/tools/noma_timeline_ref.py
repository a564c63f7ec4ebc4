"""numpy restatement of NOMA.c's timeline per sector (include/prach.h, prach_noma_timeline) in int64, written from the prose of the header on the menu's
restatement in noma_census_ref.py (classes, values, arrivals), not from the C.  It takes the 16 int32 words a NOMA.c trial logs per UE, the arrival schedule and
E as data, so a test can hand it the oracle's UEs, the product's logs or synthetic records.  Shared by tests/test_noma_timeline_cpu.py,
tests/test_noma_timeline_cases_cpu.py and the GPU tests.  No GPU, no package import."""
import numpy as np

import noma_census_ref as N

SERIES = ("arrivals", "served", "dropped", "sojourn_sum", "timer_sum", "done")
ARRIVALS, SERVED, DROPPED, SOJOURN_SUM, TIMER_SUM, DONE = range(6)
SCALARS = ("trials", "ues", "idle", "served", "dropped", "pending", "undefined", "restarted", "arrival_overflow", "done_overflow", "sojourn_sum", "timer_sum", "done_max")


def empty(ngroups, bins):
    sc = {f: np.zeros(ngroups, dtype=np.int64) for f in SCALARS}
    sc["done_max"][:] = -1
    return {"series": np.zeros((6, ngroups, 6, bins), dtype=np.int64), "scalars": sc}


def add_trial(t, g, a, sched, access_time, E, bins, bin_ms):
    sc, ser = t["scalars"], t["series"]
    cls = N.classes(a)
    val = lambda f: N.values(f, a, sched, access_time, E)
    sec, sj, tm, c, at, lost = val("sector"), val("sojourn"), val("timer"), val("completion"), val("arrival"), val("lost")
    sc["trials"][g] += 1
    sc["ues"][g] += len(a)
    for name, bit in (("idle", N.IDLE), ("served", N.SERVED), ("dropped", N.DROPPED), ("pending", N.PENDING)):
        sc[name][g] += int((cls == bit).sum())
    arrived, served, dropped = cls != N.IDLE, cls == N.SERVED, cls == N.DROPPED
    undefined = arrived & ((sec < 0) | (sec > 5) | (served & ((sj < 0) | (tm < 0) | (c < 0))))
    sc["undefined"][g] += int(undefined.sum())
    ok = arrived & ~undefined
    ab, db = at // bin_ms, c // bin_ms
    inb = ok & (ab < bins)
    np.add.at(ser[ARRIVALS, g], (sec[inb], ab[inb]), 1)
    sc["arrival_overflow"][g] += int((ok & ~inb).sum())
    m = inb & dropped
    np.add.at(ser[DROPPED, g], (sec[m], ab[m]), 1)
    s = ok & served
    sc["sojourn_sum"][g] += int(sj[s].sum())
    sc["timer_sum"][g] += int(tm[s].sum())
    sc["restarted"][g] += int((s & (lost > 0)).sum())
    if s.any():
        sc["done_max"][g] = max(int(sc["done_max"][g]), int(c[s].max()))
    m = s & inb
    np.add.at(ser[SERVED, g], (sec[m], ab[m]), 1)
    np.add.at(ser[SOJOURN_SUM, g], (sec[m], ab[m]), sj[m])
    np.add.at(ser[TIMER_SUM, g], (sec[m], ab[m]), tm[m])
    m = s & (db < bins)
    np.add.at(ser[DONE, g], (sec[m], db[m]), 1)
    sc["done_overflow"][g] += int((s & ~(db < bins)).sum())


def timeline(arrays, scheds, access_times, ends, bins, bin_ms, groups=None, ngroups=None):
    """The timelines of the trials `arrays` (int32 [nUE, 16] each): {"series": int64 [6, ngroups, 6, bins], "scalars": {field: int64 [ngroups]}}."""
    grp = list(range(len(arrays))) if groups is None else [int(g) for g in groups]
    t = empty(ngroups if ngroups is not None else max(grp) + 1, bins)
    for a, sched, at, E, g in zip(arrays, scheds, access_times, ends, grp):
        add_trial(t, g, a, sched, at, E, bins, bin_ms)
    return t


def identity(t):
    """sum(arrivals) + arrival_overflow + undefined == served + dropped + pending, per group."""
    sc = t["scalars"] if isinstance(t, dict) else t.scalars
    ser = t["series"] if isinstance(t, dict) else t.series
    left = ser[ARRIVALS].astype(np.int64).sum(axis=(1, 2)) + sc["arrival_overflow"] + sc["undefined"]
    return np.array_equal(left, sc["served"] + sc["dropped"] + sc["pending"]) and np.array_equal(sc["idle"] + sc["served"] + sc["dropped"] + sc["pending"], sc["ues"])


def same(pkg_timeline, t):
    """A package NomaTimeline against a timeline() result: every bin and every scalar."""
    return np.array_equal(pkg_timeline.series.astype(np.int64), t["series"]) and all(np.array_equal(pkg_timeline.scalars[f], t["scalars"][f]) for f in SCALARS)


def describe(t):
    sc = t["scalars"] if isinstance(t, dict) else t.scalars
    ser = t["series"] if isinstance(t, dict) else t.series
    return {**{f: sc[f].tolist() for f in SCALARS}, **{SERIES[q]: int(ser[q].astype(np.int64).sum()) for q in range(6)}}
