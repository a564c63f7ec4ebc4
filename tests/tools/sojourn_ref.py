"""numpy restatement of the sojourn histograms by arrival row (include/prach.h, prach_sojourn) over per-UE arrays, shared by tests/test_sojourn_cpu.py
and tests/test_gpu_sojourn.py.  Built on timeline_ref.per_ue: arrival time, arrived, successful and completion are the timeline's.  int64 throughout, one
flattened bincount per array.  No GPU, no package import."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timeline_ref as T  # noqa: E402


def sojourns(a, sched, access_time):
    """(arrival time, arrived, successful, sojourn c(i) - a(i)) of every UE; the sojourn of an unsuccessful UE means nothing."""
    at, arrived, ok, done = T.per_ue(a, sched, access_time)
    return at.astype(np.int64), arrived, ok, done - at.astype(np.int64)


def add_trial(sj, g, a, sched, access_time):
    """Adds one trial (int32 [nUE, 16]) to group g of the package's Sojourn `sj`."""
    rows, rw, bins, bw = sj.arrival_bins, sj.arrival_bin_ms, sj.delay_bins, sj.delay_bin_ms
    at, arrived, ok, soj = sojourns(a, sched, access_time)
    r, d = at // rw, soj // bw
    inrow = r < rows
    sj.row_arrived[g] += np.bincount(r[arrived & inrow], minlength=rows).astype(np.uint64)
    cell = ok & inrow & (d < bins)
    sj.hist[g] += np.bincount(r[cell] * bins + d[cell], minlength=rows * bins).reshape(rows, bins).astype(np.uint64)
    sj.row_delay_overflow[g] += np.bincount(r[ok & inrow & (d >= bins)], minlength=rows).astype(np.uint64)
    sc = sj.scalars
    sc["trials"][g] += 1
    sc["ues"][g] += len(a)
    sc["arrived"][g] += int(arrived.sum())
    sc["success"][g] += int(ok.sum())
    sc["restarted"][g] += int((at + soj - a[:, T.TIMER] != at)[ok].sum())
    sc["arrival_overflow"][g] += int((arrived & ~inrow).sum())
    sc["delay_overflow"][g] += int((ok & (d >= bins)).sum())
    sc["sojourn_sum"][g] += int(soj[ok].sum())
    if ok.any():
        sc["sojourn_max"][g] = max(int(sc["sojourn_max"][g]), int(soj[ok].max()))


def numpy_sojourn(pkg, arrays, scheds, access_times, spec, groups=None, ngroups=None):
    """spec = (arrival_bins, arrival_bin_ms, delay_bins, delay_bin_ms)."""
    n = len(arrays)
    grp = list(range(n)) if groups is None else list(groups)
    sj = pkg.Sojourn(ngroups if ngroups is not None else max(grp) + 1, *spec)
    for a, sched, at, g in zip(arrays, scheds, access_times, grp):
        add_trial(sj, g, a, sched, at)
    return sj


def rank_quantile(values, q, width, bins):
    """The rule of prach_sojourn_quantile on raw sojourns: the lower edge of the bin of the max(1, ceil(q n))-th smallest; -1 if none or in the overflow."""
    v = np.sort(np.asarray(values, dtype=np.int64))
    if len(v) == 0:
        return -1
    k = min(len(v), max(1, int(np.ceil(q * len(v)))))
    b = int(v[k - 1]) // width
    return b * width if b < bins else -1


def describe(sj):
    return {f: sj.scalars[f].tolist() for f in sj.scalars}
