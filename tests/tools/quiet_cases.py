"""The cases of the quiet-subframe path of prach::lcluster_kernel (prach_lcluster.hip: `quiet`), from the oracle's census alone.

Behind S3/S4 the kernel tells three kinds of subframe apart, and each must occur often enough in a test trial for a run of it to mean anything:

  taken      calls > 0 and none of them a singleton (where no call event was gathered the resolver chain is skipped: wavefront 0 adds the counters)
  offsingle  a singleton call in a subframe with t % accessTime != 1: no arrival calls there, so the subframe is quiet by its events, but a matched UE
             left alone in its bucket calls — the branch must fall through to the general path (singleton list, grant selection)
  nocall     no call at all

A base is (name, nUE, overrides); a trial of it (variant, nUE, overrides, rng, SEED) as tests/tools/trace_ref.py takes it.  Plain data and the census:
no GPU, no package import.  tests/test_lcluster_quiet_cases_cpu.py asserts the counts; tests/tools/gpu_lcluster_quiet.py runs the trials on the GPU."""
import numpy as np

import trace_ref

SEED = 700
BASES = [
    ("at7_g3_2500", 2500, dict(accessTime=7, nGrantUL=3, nPreamble=20, backoff=10)),
    ("g3_p8_3000", 3000, dict(nGrantUL=3, nPreamble=8)),
]
BASE = {name: (n, kw) for name, n, kw in BASES}
CUTS = 64  # consecutive cuts from the first subframe with an off-slot singleton


def trial(name, variant, rng):
    n, kw = BASE[name]
    return (variant, n, dict(kw), rng, SEED)


def classes(case):
    """dict(taken, offsingle, nocall: boolean arrays per subframe; calls, singles, off; steps) of one trial's uncut oracle run."""
    v, n, kw, r, s = case
    calls, singles, res = trace_ref.census(case)
    aT = kw.get("accessTime", 5)
    off = (np.arange(len(calls)) % aT) != 1
    return dict(taken=(calls > 0) & (singles == 0), offsingle=(singles > 0) & off, nocall=calls == 0, calls=calls, singles=singles, off=off,
                steps=int(res.steps), nPreamble=kw.get("nPreamble", 54))


def cuts_of(case):
    """max_steps of the CUTS consecutive cuts whose LAST subframes are t0 .. t0 + CUTS - 1, t0 the first subframe with an off-slot singleton."""
    c = classes(case)
    t0 = int(np.argmax(c["offsingle"]))
    assert c["offsingle"][t0] and t0 + CUTS <= c["steps"], (t0, c["steps"])
    return [t0 + 1 + k for k in range(CUTS)]


def taken_cuts_of(case):
    """The same from the first subframe in which the path is taken (calls, no singleton): early in a trial the window of cuts_of holds none."""
    c = classes(case)
    t1 = int(np.argmax(c["taken"]))
    assert c["taken"][t1] and t1 + CUTS <= c["steps"], (t1, c["steps"])
    return [t1 + 1 + k for k in range(CUTS)]


def all_cuts_of(case):
    return sorted(set(cuts_of(case)) | set(taken_cuts_of(case)))
