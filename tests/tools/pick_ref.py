"""numpy restatement of the pick (include/prach.h, prach_pick) over per-UE arrays, shared by tests/test_pick_cpu.py, tests/test_pick_cases_cpu.py and the
GPU tests: the predicate on xtab_ref.values, the order by np.lexsort on key and index.  It takes the arrival schedule and E as data, so a test can hand it
the oracle's, the product's or synthetic ones.  No GPU, no package import."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeline_ref as T  # noqa: E402
import xtab_ref as X  # noqa: E402

BY_INDEX, LARGEST, SMALLEST = 0, 1, 2
HEADER = ("status", "nUE", "selected", "matched", "stored", "undefined", "range_errors", "threshold", "ties_left_out")


def masks(a, sched, access_time, E, where, order, key, who):
    """(matched, undefined, key values) of every UE: a clause fails on a defined value outside lo .. hi; a UE that needs an undefined value and of which no
    clause fails is undefined; the others of the selected classes match."""
    sel = (X.classes(a) & who) != 0
    fails, undef = np.zeros(len(a), bool), np.zeros(len(a), bool)
    for f, lo, hi in where:
        v = X.values(f, a, sched, access_time, E)
        undef |= v < 0
        fails |= (v >= 0) & ((v < lo) | (v > hi))
    keyv = X.values(key, a, sched, access_time, E) if order != BY_INDEX else np.zeros(len(a), dtype=np.int64)
    undef |= keyv < 0
    return sel & ~fails & ~undef, sel & ~fails & undef, keyv, sel


def numpy_pick(a, sched, access_time, E, where, order, key, k, who):
    """The header (a dict over HEADER) and the rows (int32 [stored, 18]: the 16 logged fields, arrival, key) of one trial (int32 [nUE, 16])."""
    match, und, keyv, sel = masks(a, sched, access_time, E, where, order, key, who)
    idx = np.flatnonzero(match)
    if order == LARGEST:
        idx = idx[np.lexsort((idx, -keyv[idx]))]
    elif order == SMALLEST:
        idx = idx[np.lexsort((idx, keyv[idx]))]
    top, rest = idx[:k], idx[k:]
    at = np.asarray(T.per_ue(a, sched, access_time)[0], dtype=np.int64)
    arrival = np.where(a[top, T.ACTIVE] == -1, -1, at[top])
    keyed = order != BY_INDEX and len(top) > 0
    thr = int(keyv[top[-1]]) if keyed else -1
    hdr = dict(status=0, nUE=len(a), selected=int(sel.sum()), matched=len(idx), stored=len(top), undefined=int(und.sum()), range_errors=0, threshold=thr,
               ties_left_out=int((keyv[rest] == thr).sum()) if keyed else 0)
    rows = np.concatenate([a[top].astype(np.int64), arrival[:, None], keyv[top][:, None]], axis=1).astype(np.int32).reshape(len(top), 18)
    return hdr, rows


def rows_of(pk, t):
    """Trial t of a package Pick as (header dict, int32 [k, 18] rows in the columns of numpy_pick)."""
    r = pk.rows[t]
    names = [n for n in r.dtype.names if n != "pad"]
    assert len(names) == 18 and not r["pad"].any()
    return {f: int(pk.headers[f][t]) for f in HEADER}, np.stack([r[n] for n in names], axis=1)


def differences(pk, t, hdr, rows):
    """None when trial t of `pk` equals the reference, else what differs, as text."""
    h, r = rows_of(pk, t)
    if h != hdr:
        return f"trial {t} header {h} != {hdr}"
    if not np.array_equal(r[:len(rows)], rows):
        bad = np.argwhere(r[:len(rows)] != rows)[:4].tolist()
        return f"trial {t} rows differ at (row, column) {bad}: {[(int(r[i, j]), int(rows[i, j])) for i, j in bad]}"
    if r[len(rows):].any():
        return f"trial {t}: rows behind `stored` are not zero"
    return None


def check(pk, refs):
    """Every trial of `pk` equals refs[t] = (header, rows)."""
    assert len(pk.headers) == len(refs)
    for t, (hdr, rows) in enumerate(refs):
        d = differences(pk, t, hdr, rows)
        assert d is None, d
