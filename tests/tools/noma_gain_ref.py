"""numpy restatement of NOMA.c's near-far profile (include/prach.h, prach_noma_gain) in int64, written from the prose of the header on the menu's restatement in
noma_census_ref.py (classes, values, arrivals), not from the C.  It takes the 16 int32 words a NOMA.c trial logs per UE, the arrival schedule, E and the per-UE
gain LEVELS as data, so a test can hand it the oracle's UEs, the product's logs or synthetic records and levels.  The level of a gain is restated too
(level_of).  Shared by tests/test_noma_gain_cpu.py, tests/test_noma_gain_cases_cpu.py and the GPU tests.  No GPU, no package import."""
import numpy as np

import noma_census_ref as N

SERIES = ("arrived", "served", "dropped", "sojourn_sum", "lost_sum", "ptc_sum")
ARRIVED, SERVED, DROPPED, SOJOURN_SUM, LOST_SUM, PTC_SUM = range(6)
SCALARS = ("trials", "ues", "idle", "served", "dropped", "pending", "undefined", "below", "above", "restarted", "sojourn_sum", "lost_sum", "ptc_sum", "defined",
           "level_max", "neg_level_max")
NO_LEVEL = -2 ** 31


def level_of(lgain):
    """floor(1000.0 * lgain) per element, the product one float64 multiplication; NO_LEVEL for a non-finite lgain or |1000 lgain| >= 2^30.  int64 array."""
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.float64(1000.0) * np.asarray(lgain, dtype=np.float64)
    ok = np.isfinite(p) & (np.abs(p) < 2.0 ** 30)
    out = np.full(p.shape, NO_LEVEL, dtype=np.int64)
    out[ok] = np.floor(p[ok]).astype(np.int64)
    return out


def empty(ngroups, bins):
    sc = {f: np.zeros(ngroups, dtype=np.int64) for f in SCALARS}
    sc["level_max"][:] = -1
    sc["neg_level_max"][:] = -1
    return {"series": np.zeros((6, ngroups, 6, bins), dtype=np.int64), "scalars": sc}


def add_trial(t, g, a, sched, access_time, E, level, bins, width, lo):
    sc, ser = t["scalars"], t["series"]
    cls = N.classes(a)
    val = lambda f: N.values(f, a, sched, access_time, E)
    sec, sj, lost, ptc = val("sector"), val("sojourn"), val("lost"), val("ptc")
    L = np.asarray(level, dtype=np.int64)
    assert L.shape == (len(a),)
    sc["trials"][g] += 1
    sc["ues"][g] += len(a)
    for name, bit in (("idle", N.IDLE), ("served", N.SERVED), ("dropped", N.DROPPED), ("pending", N.PENDING)):
        sc[name][g] += int((cls == bit).sum())
    arrived, served, dropped = cls != N.IDLE, cls == N.SERVED, cls == N.DROPPED
    undefined = arrived & ((sec < 0) | (sec > 5) | (L == NO_LEVEL) | (served & ((sj < 0) | (lost < 0) | (ptc < 0))))
    sc["undefined"][g] += int(undefined.sum())
    ok = arrived & ~undefined
    had = int(sc["defined"][g]) > 0
    sc["defined"][g] += int(ok.sum())
    if ok.any():
        sc["level_max"][g] = max(int(sc["level_max"][g]), int(L[ok].max())) if had else int(L[ok].max())
        sc["neg_level_max"][g] = max(int(sc["neg_level_max"][g]), int((-L[ok]).max())) if had else int((-L[ok]).max())
    hi = int(lo) + int(bins) * int(width)  # (python integers: no overflow)
    below, above = ok & (L < lo), ok & (L >= hi)
    sc["below"][g] += int(below.sum())
    sc["above"][g] += int(above.sum())
    inb = ok & ~below & ~above
    b = np.where(inb, (L - lo) // width, 0)
    np.add.at(ser[ARRIVED, g], (sec[inb], b[inb]), 1)
    m = inb & dropped
    np.add.at(ser[DROPPED, g], (sec[m], b[m]), 1)
    s = ok & served
    sc["sojourn_sum"][g] += int(sj[s].sum())
    sc["lost_sum"][g] += int(lost[s].sum())
    sc["ptc_sum"][g] += int(ptc[s].sum())
    sc["restarted"][g] += int((s & (lost > 0)).sum())
    m = s & inb
    np.add.at(ser[SERVED, g], (sec[m], b[m]), 1)
    np.add.at(ser[SOJOURN_SUM, g], (sec[m], b[m]), sj[m])
    np.add.at(ser[LOST_SUM, g], (sec[m], b[m]), lost[m])
    np.add.at(ser[PTC_SUM, g], (sec[m], b[m]), ptc[m])


def profile(arrays, scheds, access_times, ends, levels, bins, width, lo, groups=None, ngroups=None):
    """The profiles of the trials `arrays` (int32 [nUE, 16] each) with the levels `levels` ([nUE] each):
    {"series": int64 [6, ngroups, 6, bins], "scalars": {field: int64 [ngroups]}}."""
    grp = list(range(len(arrays))) if groups is None else [int(g) for g in groups]
    t = empty(ngroups if ngroups is not None else max(grp) + 1, bins)
    for a, sched, at, E, lv, g in zip(arrays, scheds, access_times, ends, levels, grp):
        add_trial(t, g, a, sched, at, E, lv, bins, width, lo)
    return t


def _parts(t):
    return (t["series"], t["scalars"]) if isinstance(t, dict) else (t.series, t.scalars)


def identity(t):
    """sum(arrived) + below + above + undefined == served + dropped + pending, the classes add up to ues, sum(arrived) + below + above == defined; per group."""
    ser, sc = _parts(t)
    binned = ser[ARRIVED].astype(np.int64).sum(axis=(1, 2))
    return np.array_equal(binned + sc["below"] + sc["above"] + sc["undefined"], sc["served"] + sc["dropped"] + sc["pending"]) and \
        np.array_equal(sc["idle"] + sc["served"] + sc["dropped"] + sc["pending"], sc["ues"]) and np.array_equal(binned + sc["below"] + sc["above"], sc["defined"])


def same(x, t):
    """None when two profiles (package NomaGain or profile() results) are equal in every bin and every scalar, else the first few differences as text."""
    (a, asc), (b, bsc) = _parts(x), _parts(t)
    a, b = a.astype(np.int64), b.astype(np.int64)
    if a.shape != b.shape:
        return f"series: shapes {a.shape} {b.shape}"
    out = [f"{SERIES[at[0]]}{list(map(int, at[1:]))}: {int(a[tuple(at)])} != {int(b[tuple(at)])}" for at in np.argwhere(a != b)[:6]]
    for f in SCALARS:
        for (g,) in np.argwhere(np.asarray(asc[f]) != np.asarray(bsc[f]))[:6]:
            out.append(f"{f}[{g}]: {int(asc[f][g])} != {int(bsc[f][g])}")
    return "; ".join(out) or None


def describe(t):
    ser, sc = _parts(t)
    return {**{f: np.asarray(sc[f]).tolist() for f in SCALARS}, **{SERIES[q]: int(ser[q].astype(np.int64).sum()) for q in range(6)}}
