"""The routes and cases of the per-subframe preamble trace on the GPU (tests/test_gpu_trace.py; tests/tools/gpu_trace_routes.py runs the same under another
library build).  A route pins one WRITER of the trace rows with the engine options and prach_timing fields tests/tools/kernel_matrix.py uses; a trace call
takes the paths engine option fast = 0 takes, so four workgroups per trial land on prach::cluster_kernel, never on the lean kernel (rec_mode 3).  Every
comparison is with tests/tools/trace_ref.py (the oracle), never with another call of the library."""
import numpy as np

import trace_ref as TR

DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0, lds_records=1, trace_scheme=1)  # (every option a route sets, at the engine's defaults)

# name -> (RNG mode, engine options, prach_timing fields every call must report, rec_mode the call must NOT report or None)
ROUTES = {
    "batch_w8_philox": (1, dict(cluster=1, batch_waves=8), dict(rec_mode=4, cluster_size=1), None),
    "batch_w16_philox": (1, dict(cluster=1, batch_waves=16), dict(rec_mode=4, cluster_size=1), None),
    "cluster1_glibc": (0, dict(cluster=1), dict(rec_mode=4, cluster_size=1), None),  # one workgroup per trial in the reference's stream: batch_kernel<16, true>
    "cluster_wide_glibc": (0, dict(cluster=1, wide_records=1), dict(rec_mode=0, cluster_size=1), None),
    "cluster4_philox": (1, dict(cluster=4), dict(rec_mode=2, cluster_size=4), 3),  # LDS records on the general kernel: the lean kernel is off for trace calls
    "cluster4_global_philox": (1, dict(cluster=4, lds_records=0), dict(rec_mode=0, cluster_size=4), 3),
    "legacy_philox": (1, dict(legacy=1), dict(cluster_size=0), None),
}

# (name, nUE, overrides), each for both variants.  over_3000: up to 61 calls per subframe, all five residues of t % 5 occur.
CASES = [
    ("over_3000", 3000, dict(maxMsg2TxCount=3, nGrantUL=4)),
    ("corner_1500", 1500, dict(maxMsg2TxCount=0, nGrantUL=1, maxRarWindow=1)),
    ("p8_at1", 4000, dict(nPreamble=8, backoff=5, nGrantUL=12, maxRarWindow=2, maxMsg2TxCount=1, accessTime=1)),
    ("default_1", 1, {}),
    ("default_65", 65, {}),
]
SECTOR = ("sector", 3000, dict(nGrantUL=3, sector_grants=1))  # RandomAccessWithNOMA.c with PRACH_FLAG_SECTOR_GRANTS: batch_kernel, or trial_kernel where a route rules it out
EVERY = ("every_600", 600, dict(maxMsg2TxCount=0, nGrantUL=1, max_steps=1500))  # RandomAccessWithNOMA.c, pinned at EVERY subframe by prefix runs


def route_cases(route, names=None):
    """The trace_ref cases (variant, nUE, overrides, rng, seed) of a route's call; the reference-stream route with one workgroup per trial takes four seeds
    of over_3000."""
    rng = ROUTES[route][0]
    out = []
    for k, (name, n, kw) in enumerate(CASES):
        if names and name not in names:
            continue
        for v in (0, 1):
            seeds = [100 * k + v] + ([100 * k + v + 10 * j for j in (1, 2, 3)] if route == "cluster1_glibc" and name == "over_3000" else [])
            out += [(v, n, kw, rng, s) for s in seeds]
    return out


def lib_cfg(pkg, case):
    v, n, kw, r, s = case
    return pkg.make_cfg(n, variant=v, rng_mode=r, seed=s, **TR.lib_overrides(kw))


def set_route(eng, route):
    for k, v in DEFAULTS.items():
        eng.set(k, v)
    for k, v in ROUTES[route][1].items():
        eng.set(k, v)


def reset(eng):
    for k, v in DEFAULTS.items():
        eng.set(k, v)
    eng.set("mem_budget_mb", 1 << 20)  # (more than any device has: one launch)


def pin_failure(route, tm):
    _, _, pin, never = ROUTES[route]
    want = dict(pin, fallback_trials=0, trial_kernel_reruns=0)
    got = {k: getattr(tm, k) for k in want}
    if never is not None and tm.rec_mode == never:
        return f"rec_mode {never}: the lean kernel ran a trace call"
    return None if got == want else f"prach_timing {got}, the route pins {want}"


def series_of(tr, g):
    return [tr.series[n][g].astype(np.int64) for n in ("calls", "singles", "txop", "collisions")]


def check_per_subframe(pkg, eng, cases, refs, pin=None):
    """One trace call (bin_ms = 1, group = NULL, logs of every trial) over `cases` and the plain call of the same cfgs; returns (failure texts, the trace
    call's prach_timing).  refs[k]: the trace_ref.Ref of cases[k]."""
    cfgs = [lib_cfg(pkg, c) for c in cases]
    bins = max(60000 if c[2].get("uniform") else 10000 for c in cases)
    res, logs, tr = eng.run_trials_trace(cfgs, bins, 1, want_logs=True)
    tm = eng.timing()
    bad = []
    if pin:
        pf = pin_failure(pin, tm)
        if pf:
            bad.append(pf)
    if not (tm.trace_ms > 0 and tm.summary_ms == 0 and tm.dist_ms == 0 and tm.timeline_ms == 0 and tm.sojourn_ms == 0):
        bad.append(f"timing: trace_ms {tm.trace_ms}, others {tm.summary_ms} {tm.dist_ms} {tm.timeline_ms} {tm.sojourn_ms}")
    pres, plogs = eng.run_trials(cfgs, want_logs=True)
    if eng.timing().trace_ms != 0:
        bad.append("trace_ms != 0 after a plain call")
    for g, c in enumerate(cases):
        r = refs[g]
        where = f"{c}: "
        calls, singles, txop, coll = series_of(tr, g)
        bad += TR.check_trace(r, calls, singles, txop, coll, where)
        sc = {f: int(tr.scalars[f][g]) for f in tr.scalars}
        exp = dict(trials=1, subframes=r.steps, calls=int(r.calls.sum()), singles=int(r.singles.sum()), txop=res[g].totalPreambleTxop,
                   collisions=res[g].collisionPreambles, overflow_calls=0, calls_max=int(r.calls.max()) if r.steps else -1)
        if sc != exp:
            bad.append(f"{where}scalars {sc} != {exp}")
        if (int(txop.sum()), int(coll.sum())) != (res[g].totalPreambleTxop, res[g].collisionPreambles) or \
                (res[g].totalPreambleTxop, res[g].collisionPreambles, res[g].steps) != (r.res.totalPreambleTxop, r.res.collisionPreambles, r.res.steps):
            bad.append(f"{where}sums {int(txop.sum())} {int(coll.sum())}, prach_result {res[g].totalPreambleTxop} {res[g].collisionPreambles} steps {res[g].steps}, "
                       f"oracle {r.res.totalPreambleTxop} {r.res.collisionPreambles} steps {r.res.steps}")
        if bytes(res[g]) != bytes(pres[g]) or bytes(logs[g]) != bytes(plogs[g]):
            bad.append(f"{where}results or logs differ from the plain call's")
    return bad, tm
