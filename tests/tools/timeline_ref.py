"""numpy restatement of the timelines (include/prach.h, prach_timeline) over per-UE arrays, shared by tests/test_timeline_cpu.py and
tests/test_gpu_timeline.py.  It takes the arrival schedule as data, so a test can hand it the oracle's, the product's or a synthetic one; the arithmetic is
reduce_cases.timeline_add.  No GPU, no package import."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reduce_cases import arrival_times, timeline_add  # noqa: E402

TIMER, ACTIVE, TXTIME, FLAG = 1, 2, 3, 14  # columns of the 16-field per-UE log
SERIES = ("arrivals", "success", "sojourn_sum", "timer_sum", "done")


def as_array(log):
    return np.frombuffer(log, dtype=np.int32).reshape(-1, 16)


def oracle_cfg(ob, c, **kw):
    """The oracle's form of a product config (Beta.c / RandomAccessWithNOMA)."""
    return ob.make_cfg(c.nUE, variant=c.variant, uniform=c.uniform, nPreamble=c.nPreamble, backoff=c.backoff, nGrantUL=c.nGrantUL, maxRarWindow=c.maxRarWindow,
                       maxMsg2TxCount=c.maxMsg2TxCount, accessTime=c.accessTime, max_steps=c.max_steps, **kw)


def per_ue(a, sched, access_time):
    """(arrival time a(i), arrived, successful, completion c(i)) of every UE: a(i) = accessTime x the first slot s with sched[s] > i."""
    return arrival_times(len(a), sched, access_time), a[:, ACTIVE] != -1, (a[:, FLAG] == 1) & (a[:, ACTIVE] != -1), a[:, TXTIME].astype(np.int64) + 6


def add_trial(tl, g, a, sched, access_time):
    """Adds one trial (int32 [nUE, 16]) to group g of the package's Timeline `tl`, in numpy (reduce_cases.timeline_add: int64 throughout)."""
    timeline_add(tl.series, tl.scalars, g, a, sched, access_time, tl.bins, tl.bin_ms)


def numpy_timeline(pkg, arrays, scheds, access_times, bins, width, groups=None, ngroups=None):
    n = len(arrays)
    grp = list(range(n)) if groups is None else list(groups)
    tl = pkg.Timeline(ngroups if ngroups is not None else max(grp) + 1, bins, width)
    for a, sched, at, g in zip(arrays, scheds, access_times, grp):
        add_trial(tl, g, a, sched, at)
    return tl


def describe(tl):
    return {f: tl.scalars[f].tolist() for f in tl.scalars}
