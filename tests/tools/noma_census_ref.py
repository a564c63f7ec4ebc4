"""numpy restatement of THE NOMA MENU (include/prach.h: classes, fields, census table, columns) over per-UE arrays, written from the prose of the header, not
from the C.  It takes the 16 int32 words a NOMA.c trial logs per UE — the oracle's noma_ue words are the same 16 — the arrival schedule and E as data, so a test
can hand it the oracle's UEs, the product's logs or synthetic records.  Shared by tests/test_noma_census_cpu.py, tests/test_noma_census_cases_cpu.py and the
GPU tests.  No GPU, no package import."""
import numpy as np

SERVED, PENDING, IDLE, DROPPED = 1, 2, 4, 8
ALL = SERVED | PENDING | IDLE | DROPPED
FIELD_NAMES = ("one", "arrival", "sojourn", "completion", "timer", "ptc", "retx", "msg3fail", "age", "state", "sector", "preamble", "lost")
ONE, ARRIVAL, SOJOURN, COMPLETION, TIMER, PTC, RETX, MSG3FAIL, AGE, STATE, SECTOR, PREAMBLE, LOST = range(13)
# columns of the 16-word record
W_TIMER, W_ACTIVE, W_TXTIME, W_NOWBACKOFF, W_PREAMBLE, W_SECTOR, W_RETX, W_PTC, W_MSG3WAIT, W_RA, W_FAIL = 1, 2, 3, 6, 7, 8, 10, 11, 13, 14, 15
SCALARS = ("trials", "ues", "idle", "served", "dropped", "pending", "selected", "binned", "undefined", "row_sum", "col_sum", "row_max", "col_max")
RAW = 16


def field_id(f):
    return FIELD_NAMES.index(f.lower()) if isinstance(f, str) else int(f)


def as_array(ues):
    """The oracle's NomaUE array (16 int32 + a double) or a product log (16 int32) as int32 [nUE, 16]."""
    b = np.frombuffer(ues, dtype=np.uint8)
    n = len(ues)
    return b.reshape(n, -1)[:, :64].copy().view(np.int32).reshape(n, 16)


def arrivals(n, sched, access_time):
    """a(i): access_time x the first slot s with sched[s] > i; a UE no slot activates gets access_time x the number of slots."""
    return np.int64(access_time) * np.searchsorted(np.asarray(sched, dtype=np.int64), np.arange(n, dtype=np.int64), side="right").astype(np.int64)


def classes(a):
    a = a.astype(np.int64)
    idle = a[:, W_SECTOR] == -1
    served = ~idle & (a[:, W_RA] == 1)
    dropped = ~idle & ~served & ((a[:, W_FAIL] & 0xffff) != 0)
    return np.where(idle, IDLE, np.where(served, SERVED, np.where(dropped, DROPPED, PENDING)))


def states(a, E):
    cls = classes(a)
    a = a.astype(np.int64)
    act, nb, tx, m3 = a[:, W_ACTIVE], a[:, W_NOWBACKOFF], a[:, W_TXTIME], a[:, W_MSG3WAIT]
    pend = np.full(len(a), 8, dtype=np.int64)
    pend[(act == 1) & (nb > 0)] = 3
    pend[(act == 1) & (nb <= 0) & (tx >= E)] = 4
    pend[(act == 1) & (nb <= 0) & (tx < E)] = 5
    pend[(act == 2) & (m3 == 0)] = 6
    pend[(act == 2) & (m3 != 0)] = 7
    return np.where(cls == IDLE, 0, np.where(cls == SERVED, 1, np.where(cls == DROPPED, 2, pend))).astype(np.int64)


def values(field, a, sched, access_time, E):
    """The value of `field` for every UE as int64; negative: UNDEFINED."""
    field = field_id(field)
    cls = classes(a)
    w = a.astype(np.int64)
    n = len(a)
    at = arrivals(n, sched, access_time)
    arrived, served = cls != IDLE, cls == SERVED
    und = np.full(n, -1, dtype=np.int64)
    c = w[:, W_TXTIME] + 6
    if field == ONE:
        return np.zeros(n, dtype=np.int64)
    if field == STATE:
        return states(a, E)
    if field == LOST:  # SOJOURN - TIMER, undefined where either is
        sj, tm = c - at, w[:, W_TIMER]
        return np.where(served & (sj >= 0) & (tm >= 0), sj - tm, und)
    v, ok = {ARRIVAL: (at, arrived), SOJOURN: (c - at, served), COMPLETION: (c, served), TIMER: (w[:, W_TIMER], arrived), PTC: (w[:, W_PTC], arrived),
             RETX: (w[:, W_RETX], arrived), MSG3FAIL: (w[:, W_FAIL] >> 16, arrived), AGE: (np.int64(E) - at, arrived), SECTOR: (w[:, W_SECTOR], arrived),
             PREAMBLE: (w[:, W_PREAMBLE], arrived)}[field]
    return np.where(ok, v, und)


def empty(ngroups, rows, cols):
    sc = {f: np.zeros(ngroups, dtype=np.int64) for f in SCALARS}
    sc["row_max"][:] = -1
    sc["col_max"][:] = -1
    return {"cells": np.zeros((ngroups, rows[2] + 1, cols[2] + 1), dtype=np.uint64), "scalars": sc}


def add_trial(t, g, a, sched, access_time, E, rows, cols, who):
    (rf, rw, rb), (cf, cw, cb) = rows, cols
    cls = classes(a)
    sc = t["scalars"]
    sc["trials"][g] += 1
    sc["ues"][g] += len(a)
    for name, bit in (("idle", IDLE), ("served", SERVED), ("dropped", DROPPED), ("pending", PENDING)):
        sc[name][g] += int((cls == bit).sum())
    sel = (cls & who) != 0
    rv, cv = values(rf, a, sched, access_time, E), values(cf, a, sched, access_time, E)
    good = sel & (rv >= 0) & (cv >= 0)
    sc["selected"][g] += int(sel.sum())
    sc["binned"][g] += int(good.sum())
    sc["undefined"][g] += int((sel & ~good).sum())
    np.add.at(t["cells"][g], (np.minimum(rv[good] // rw, rb), np.minimum(cv[good] // cw, cb)), 1)
    sc["row_sum"][g] += int(rv[good].sum())
    sc["col_sum"][g] += int(cv[good].sum())
    if good.any():
        sc["row_max"][g] = max(int(sc["row_max"][g]), int(rv[good].max()))
        sc["col_max"][g] = max(int(sc["col_max"][g]), int(cv[good].max()))


def census(arrays, scheds, access_times, ends, rows, cols, who, groups=None, ngroups=None):
    """The census of the trials `arrays` (int32 [nUE, 16] each): {"cells": uint64 [ngroups, rb + 1, cb + 1], "scalars": {field: int64 [ngroups]}}."""
    rows, cols = (field_id(rows[0]), int(rows[1]), int(rows[2])), (field_id(cols[0]), int(cols[1]), int(cols[2]))
    grp = list(range(len(arrays))) if groups is None else [int(g) for g in groups]
    t = empty(ngroups if ngroups is not None else max(grp) + 1, rows, cols)
    for a, sched, at, E, g in zip(arrays, scheds, access_times, ends, grp):
        add_trial(t, g, a, sched, at, E, rows, cols, who)
    return t


def same(pkg_census, t):
    """A package NomaCensus against a census() result: every cell and every scalar."""
    return np.array_equal(pkg_census.cells, t["cells"]) and all(np.array_equal(pkg_census.scalars[f], t["scalars"][f]) for f in SCALARS)


def describe(c):
    sc = c["scalars"] if isinstance(c, dict) else c.scalars
    return {f: sc[f].tolist() for f in SCALARS}


def columns(fields, a, sched, access_time, E):
    """int32 [ncols, nUE]: the columns of one trial; a field is a menu name or id, "raw:<word>" or RAW + word."""
    out = np.empty((len(fields), len(a)), dtype=np.int32)
    for k, f in enumerate(fields):
        if isinstance(f, str) and f.startswith("raw:"):
            f = RAW + int(f[4:])
        f = field_id(f)
        if f >= RAW:
            out[k] = a[:, f - RAW]
        else:
            v = values(f, a, sched, access_time, E)
            out[k] = np.where(v < 0, -1, v).astype(np.int32)
    return out


def state_census(a, E):
    """UEs per STATE 0 .. 8."""
    return np.bincount(states(a, E), minlength=9).tolist()


def rank_quantile(vals, q, width, bins):
    """The rule of prach_xtab_quantile on raw column values: the lower edge of the bin of the max(1, ceil(q * n))-th smallest, -1 if none or in the overflow."""
    v = np.sort(np.asarray(vals, dtype=np.int64))
    if len(v) == 0:
        return -1
    rank = min(max(int(np.ceil(q * len(v))), 1), len(v))
    b = int(v[rank - 1]) // width
    return b * width if b < bins else -1
