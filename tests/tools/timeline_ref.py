"""numpy restatement of the timelines (include/prach.h, prach_timeline) over per-UE arrays, shared by tests/test_timeline_cpu.py and
tests/test_gpu_timeline.py.  It takes the arrival schedule as data, so a test can hand it the oracle's or the product's.  No GPU, no package import."""
import numpy as np

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
    slot = np.searchsorted(np.asarray(sched, dtype=np.int64), np.arange(len(a), dtype=np.int64), side="right")
    return access_time * slot, a[:, ACTIVE] != -1, (a[:, FLAG] == 1) & (a[:, ACTIVE] != -1), a[:, TXTIME].astype(np.int64) + 6


def add_trial(tl, g, a, sched, access_time):
    """Adds one trial (int32 [nUE, 16]) to group g of the package's Timeline `tl`, in numpy."""
    bins, w = tl.bins, tl.bin_ms
    at, arrived, ok, c = per_ue(a, sched, access_time)
    timer = a[:, TIMER].astype(np.int64)
    ab, db = at // w, c // w
    s, sc = tl.series, tl.scalars
    s["arrivals"][g] += np.bincount(ab[arrived & (ab < bins)], minlength=bins).astype(np.uint64)
    inb = ok & (ab < bins)
    s["success"][g] += np.bincount(ab[inb], minlength=bins).astype(np.uint64)
    s["sojourn_sum"][g] += np.bincount(ab[inb], weights=(c - at)[inb], minlength=bins).astype(np.uint64)  # (float64 sums of integers below 2^53: exact)
    s["timer_sum"][g] += np.bincount(ab[inb], weights=timer[inb], minlength=bins).astype(np.uint64)
    s["done"][g] += np.bincount(db[ok & (db < bins)], minlength=bins).astype(np.uint64)
    sc["trials"][g] += 1; sc["ues"][g] += len(a); sc["arrived"][g] += int(arrived.sum()); sc["success"][g] += int(ok.sum())
    sc["restarted"][g] += int((ok & (c - timer != at)).sum())
    sc["arrival_overflow"][g] += int((arrived & (ab >= bins)).sum()); sc["done_overflow"][g] += int((ok & (db >= bins)).sum())
    sc["sojourn_sum"][g] += int((c - at)[ok].sum()); sc["timer_sum"][g] += int(timer[ok].sum())
    if ok.any():
        sc["done_max"][g] = max(int(sc["done_max"][g]), int(c[ok].max()))


def numpy_timeline(pkg, arrays, scheds, access_times, bins, width, groups=None, ngroups=None):
    n = len(arrays)
    grp = list(range(n)) if groups is None else list(groups)
    tl = pkg.Timeline(ngroups if ngroups is not None else max(grp) + 1, bins, width)
    for a, sched, at, g in zip(arrays, scheds, access_times, grp):
        add_trial(tl, g, a, sched, at)
    return tl


def describe(tl):
    return {f: tl.scalars[f].tolist() for f in tl.scalars}
