"""The reference of the per-subframe preamble trace (prach_run_trials_trace), from the oracle alone: no call of the library under test.

  calls, singles   per subframe, from the oracle's census (oracle_set_census): both variants, both RNG modes
  txop, collisions the oracle's totalPreambleTxop / collisionPreambles of runs cut at max_steps = e are the two weighted series summed over the
                   subframes [0, e): every edge e pins a prefix sum, consecutive edges pin the sum of the stretch between them
  Beta.c           adds 1 per call to totalPreambleTxop and 1 per collided call to collisionPreambles (Beta.c:334,349-351), so there
                   txop_t = calls_t and collisions_t = calls_t - singles_t at EVERY subframe

A case is (variant, nUE, overrides, rng, seed): ob.make_cfg(nUE, variant=variant, **overrides) run on ob.Rng(rng, seed); the library's cfg of the same
trial is pkg.make_cfg(nUE, variant=variant, rng_mode=rng, seed=seed, **overrides) (lib_overrides turns the oracle's sector_grants into the flag).
The census is process-global state of the oracle: references are computed one at a time (ref() caches them)."""
import ctypes as C

import numpy as np

from oracle import binding as ob

_cache = {}


def _key(case):
    v, n, kw, r, s = case
    return (v, n, tuple(sorted(kw.items())), r, s)


def lib_overrides(kw):
    """The overrides of a case as pkg.make_cfg takes them."""
    out = dict(kw)
    if out.pop("sector_grants", 0):
        out["flags"] = 1  # PRACH_FLAG_SECTOR_GRANTS
    return out


def run(case, max_steps=None):
    """One oracle run of the case (max_steps: cut there).  Returns the OracleResult."""
    v, n, kw, r, s = case
    kw = dict(kw)
    if max_steps is not None:
        kw["max_steps"] = int(max_steps)
    res, _ = ob.run_trial(ob.make_cfg(n, variant=v, **kw), ob.Rng(r, s), want_ues=False)
    return res


def census(case):
    """(calls[steps], singles[steps], OracleResult) of the whole trial."""
    L = ob.lib()
    L.oracle_set_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.oracle_set_census.restype = None
    T = 60000 if case[2].get("uniform") else 10000
    calls, singles = np.zeros(T, np.int32), np.zeros(T, np.int32)
    L.oracle_set_census(None, singles.ctypes.data, calls.ctypes.data, T)
    try:
        res = run(case)
    finally:
        L.oracle_set_census(None, None, None, 0)
    steps = int(res.steps)
    assert not calls[steps:].any() and not singles[steps:].any()
    return calls[:steps].astype(np.int64), singles[:steps].astype(np.int64), res


def edges_of(steps, k):
    """At most k prefix edges in (0, steps], spread evenly, the last step included."""
    k = max(1, min(int(k), steps))
    return sorted({(steps * (j + 1) + k - 1) // k for j in range(k)})


class Ref:
    """calls / singles per subframe, and (edge, txop over [0, edge), collisions over [0, edge)) for every prefix edge."""

    def __init__(self, case, max_edges=16, every=False):
        self.case = case
        self.calls, self.singles, self.res = census(case)
        self.steps = len(self.calls)
        self.beta = case[0] == ob.VARIANT_BETA_C
        self.edges = list(range(1, self.steps + 1)) if every else edges_of(self.steps, max_edges)
        self.prefix = []
        for e in self.edges:
            r = self.res if e == self.steps else run(case, e)
            self.prefix.append((e, int(r.totalPreambleTxop), int(r.collisionPreambles)))
        assert self.prefix[-1][0] == self.steps

    def weighted(self):
        """Beta.c only: (txop, collisions) per subframe."""
        assert self.beta
        return self.calls, self.calls - self.singles

    def stretches(self):
        """[(lo, hi, txop over [lo, hi), collisions over [lo, hi))] between consecutive edges, from 0."""
        out, lo, px, pq = [], 0, 0, 0
        for e, x, q in self.prefix:
            out.append((lo, e, x - px, q - pq))
            lo, px, pq = e, x, q
        return out

    def check_self(self):
        """What the oracle's two views owe each other: at every edge txop - collisions of the prefix run is the census's cumulative singles (a single adds 1 to
        txop only, a collided call the same amount to both, in both programs), and for Beta.c txop is the cumulative calls.  Returns the number of mismatches."""
        cs, cc = np.cumsum(self.singles), np.cumsum(self.calls)
        bad = 0
        for e, x, q in self.prefix:
            bad += x - q != cs[e - 1]
            if self.beta:
                bad += x != cc[e - 1]
            bad += x < cc[e - 1] or q < cc[e - 1] - cs[e - 1]  # (WithNOMA weights a collided call by check >= 2)
        return int(bad)


def ref(case, max_edges=16, every=False):
    k = (_key(case), max_edges, every)
    if k not in _cache:
        _cache[k] = Ref(case, max_edges, every)
    return _cache[k]


def binned(per_subframe, bins, bin_ms):
    """(series[bins], what lies at or behind bins * bin_ms) of one per-subframe array."""
    per_subframe = np.asarray(per_subframe, dtype=np.int64)
    b = np.arange(len(per_subframe)) // bin_ms
    inside = b < bins
    out = np.zeros(bins, dtype=np.int64)
    np.add.at(out, b[inside], per_subframe[inside])
    return out, int(per_subframe[~inside].sum())


def check_trace(r, calls, singles, txop, coll, where=""):
    """One trial's trace at bin_ms = 1 (arrays of at least r.steps entries) against the reference r.  Returns a list of failure texts."""
    bad = []
    n = r.steps
    for name, got, exp in (("calls", calls, r.calls), ("singles", singles, r.singles)):
        got = np.asarray(got[:n], dtype=np.int64)
        d = np.nonzero(got != exp)[0]
        if d.size:
            bad.append(f"{where}{name}: {d.size} subframes differ, first t={d[0]}: {got[d[0]]} != census {exp[d[0]]}")
    for name, arr in (("calls", calls), ("singles", singles), ("txop", txop), ("collisions", coll)):
        if np.asarray(arr[n:]).any():
            bad.append(f"{where}{name}: non-zero behind the last subframe {n}")
    cx, cq = np.cumsum(np.asarray(txop[:n], dtype=np.int64)), np.cumsum(np.asarray(coll[:n], dtype=np.int64))
    for e, x, q in r.prefix:
        if (cx[e - 1], cq[e - 1]) != (x, q):
            bad.append(f"{where}prefix [0, {e}): txop {cx[e - 1]} collisions {cq[e - 1]} != oracle {x} {q}")
            break
    if r.beta:
        wx, wq = r.weighted()
        if not np.array_equal(np.asarray(txop[:n], dtype=np.int64), wx) or not np.array_equal(np.asarray(coll[:n], dtype=np.int64), wq):
            bad.append(f"{where}Beta.c: txop_t != calls_t or collisions_t != calls_t - singles_t at some subframe")
    return bad
