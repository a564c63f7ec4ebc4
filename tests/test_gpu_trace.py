"""prach_run_trials_trace on the GPU: the per-subframe rows every simulation kernel writes and prach::trace_kernel's reduction of them, against the oracle's
census and prefix runs (tests/tools/trace_ref.py) — never against another call of the library.  tests/tools/trace_cases.py has the routes and cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import trace_cases as TC  # noqa: E402
import trace_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng(engine):
    TC.reset(engine)
    yield engine
    TC.reset(engine)


def _refs(cases, max_edges=16, every=False):
    return [TR.ref(c, max_edges, every) for c in cases]


@pytest.mark.parametrize("route", list(TC.ROUTES))
def test_every_writer_per_subframe(pkg, eng, route):
    """1. bin_ms = 1, group = NULL: calls and singles equal the census at every subframe, the weighted series the prefix totals at every edge (Beta.c: at every
    subframe), their sums the call's own prach_result; results and logs are byte-equal to the plain call's; the route's kernel wrote the rows."""
    cases = TC.route_cases(route)
    TC.set_route(eng, route)
    bad, _ = TC.check_per_subframe(pkg, eng, cases, _refs(cases), pin=route)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("route", ["batch_w8_philox", "batch_w16_philox", "cluster1_glibc", "legacy_philox", "cluster4_philox"])
def test_sector_grants_and_every_subframe(pkg, eng, route):
    """1. (continued) the per-sector grant path (batch_kernel, or trial_kernel under `legacy`), and one small RandomAccessWithNOMA.c trial pinned at EVERY
    subframe by prefix runs."""
    rng = TC.ROUTES[route][0]
    TC.set_route(eng, route)
    name, n, kw = TC.SECTOR
    sector = [(1, n, kw, rng, 41)]
    bad, _ = TC.check_per_subframe(pkg, eng, sector, _refs(sector))
    name, n, kw = TC.EVERY
    every = [(1, n, kw, rng, 43)]
    refs = _refs(every, every=True)
    assert len(refs[0].prefix) == 1500
    bad += TC.check_per_subframe(pkg, eng, every, refs)[0]
    assert not bad, "\n".join(bad[:20])


def test_counted_once_after_a_rerun(pkg, eng):
    """2. reset_storm (Uniform, 60 000 subframes) and p3_b40_at6 leave the batch kernel by design (tests/tools/kernel_matrix.py LEAVES): the rows of the
    launch whose result is thrown away are never read.  reset_storm is also a 60 000-entry row of several tiles, and, with bins cut to 30 000, the overflow."""
    storm = (0, 2600, dict(uniform=1, nPreamble=54, backoff=5, nGrantUL=1, maxRarWindow=1, maxMsg2TxCount=0, accessTime=10), 1, 600)
    p3 = [(v, 3000, dict(nPreamble=3, backoff=40, nGrantUL=12, maxRarWindow=6, maxMsg2TxCount=3, accessTime=6), 1, 900 + v) for v in (0, 1)]
    TC.set_route(eng, "batch_w16_philox")
    cases = [storm] + p3
    refs = [TR.ref(storm, 6)] + _refs(p3)
    assert refs[0].steps == 60000 > 2 * pkg.trace_tile_subframes()
    bad, tm = TC.check_per_subframe(pkg, eng, cases, refs)
    assert tm.fallback_trials > 0, "no trial left its kernel: the case does not test a rerun"
    assert not bad, "\n".join(bad[:20])
    res, _, tr = eng.run_trials_trace([TC.lib_cfg(pkg, storm)], 30000, 1)
    assert eng.timing().fallback_trials > 0
    r = refs[0]
    calls, singles, txop, coll = TC.series_of(tr, 0)
    assert np.array_equal(calls, r.calls[:30000]) and np.array_equal(singles, r.singles[:30000])
    assert np.array_equal(txop, r.calls[:30000]) and np.array_equal(coll, (r.calls - r.singles)[:30000])  # (Beta.c)
    assert int(tr.scalars["overflow_calls"][0]) == int(r.calls[30000:].sum()) > 0
    assert int(tr.scalars["calls"][0]) == int(r.calls.sum()) and int(tr.scalars["subframes"][0]) == 60000
    assert int(tr.scalars["txop"][0]) == res[0].totalPreambleTxop == r.res.totalPreambleTxop


def _small_cases(n, seed0, rng=None):
    """n small trials of mixed size: Beta.c (all four series known per subframe) and, every fifth, RandomAccessWithNOMA.c.  rng None: both modes in turn."""
    return [((1 if k % 5 == 4 else 0), 40 + 37 * (k % 11) + (k % 3), dict(nGrantUL=2 + k % 4, maxMsg2TxCount=1 + k % 3), k % 2 if rng is None else rng, seed0 + k)
            for k in range(n)]


def _group_reference(cases, groups, ngroups, bins, bin_ms):
    """Per group: the four binned series (txop / collisions of RandomAccessWithNOMA.c trials: None is returned for a group that has one, their scalars are still
    known), the overflow of the calls, and the scalars."""
    ser = np.zeros((ngroups, 4, bins), dtype=np.int64)
    sc = [dict(trials=0, subframes=0, calls=0, singles=0, txop=0, collisions=0, overflow_calls=0, calls_max=-1) for _ in range(ngroups)]
    weighted_known = [True] * ngroups
    for c, g in zip(cases, groups):
        r = TR.ref(c, 1)
        per = [r.calls, r.singles] + (list(r.weighted()) if r.beta else [np.zeros(r.steps, np.int64)] * 2)
        weighted_known[g] = weighted_known[g] and r.beta
        for q in range(4):
            b, over = TR.binned(per[q], bins, bin_ms)
            ser[g, q] += b
            if q == 0:
                sc[g]["overflow_calls"] += over
        s = sc[g]
        s["trials"] += 1; s["subframes"] += r.steps; s["calls"] += int(r.calls.sum()); s["singles"] += int(r.singles.sum())
        s["txop"] += int(r.res.totalPreambleTxop); s["collisions"] += int(r.res.collisionPreambles)
        s["calls_max"] = max(s["calls_max"], int(r.calls.max()) if r.steps else -1)
    return ser, sc, weighted_known


def _assert_groups(tr, ser, sc, weighted_known):
    for g in range(tr.ngroups):
        got = TC.series_of(tr, g)
        for q, name in enumerate(("calls", "singles", "txop", "collisions")):
            if q >= 2 and not weighted_known[g]:
                continue
            d = np.nonzero(got[q] != ser[g, q])[0]
            assert not d.size, f"group {g} {name}: {d.size} bins differ, first bin {d[0]}: {got[q][d[0]]} != {ser[g, q][d[0]]}"
        assert {f: int(tr.scalars[f][g]) for f in tr.scalars} == sc[g], g


def test_split_launches(pkg, eng):
    """3. ~300 small trials whose arena does not fit the budget of one launch: ten groups equal the sum of the per-trial references."""
    cases = _small_cases(300, 5000, rng=1)  # (one RNG mode: the engine launches the two modes apart anyway)
    groups = [k % 10 for k in range(300)]
    ser, sc, known = _group_reference(cases, groups, 10, 10000, 1)
    eng.set("mem_budget_mb", 400)
    res, _, tr = eng.run_trials_trace([TC.lib_cfg(pkg, c) for c in cases], 10000, 1, groups=groups, ngroups=10)
    assert eng.timing().launches >= 2
    assert all(r.status == 0 for r in res)
    _assert_groups(tr, ser, sc, known)


@pytest.mark.parametrize("bin_ms,bins", [(7, 1429), (500, 20), (500, 3)])
def test_binning_under_both_schemes(pkg, eng, bin_ms, bins):
    """4. bin_ms = 7 does not divide the 5 ms grant window; 24 trials of mixed size in three groups, one of them cut by max_steps (nothing behind its
    time_exit); (500, 3) leaves subframes behind the last bin.  Scheme 0 and scheme 1 against the reference."""
    cases = _small_cases(23, 7000) + [(0, 900, dict(nGrantUL=3, max_steps=700), 1, 7100)]
    groups = [2 if c[0] == 1 else k % 2 for k, c in enumerate(cases)]  # (groups 0 and 1 are Beta.c only: all four series are known bin by bin)
    ser, sc, known = _group_reference(cases, groups, 3, bins, bin_ms)
    assert known == [True, True, False]
    assert TR.ref(cases[-1], 1).steps == 700
    if bins * bin_ms < 10000:
        assert sum(s["overflow_calls"] for s in sc) > 0
    for scheme in (0, 1):
        eng.set("trace_scheme", scheme)
        res, _, tr = eng.run_trials_trace([TC.lib_cfg(pkg, c) for c in cases], bins, bin_ms, groups=groups, ngroups=3)
        assert res[-1].time_exit == 700 and res[-1].steps == 700
        _assert_groups(tr, ser, sc, known)


def test_refusals(pkg, eng):
    """5. NOMA.c is refused before anything is launched; a bad spec, a bad group id, a NULL output give PRACH_ERR_ARG."""
    import ctypes as C
    ok = pkg.make_cfg(100, rng_mode=1)
    before = eng.timing().launches
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_trace([ok, pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=1)], 100, 1)
    assert ei.value.status == -2 and eng.timing().launches == before
    for kw in (dict(bins=0), dict(bins=pkg.TRACE_MAX_BINS + 1), dict(bin_ms=0)):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_trace([ok], kw.get("bins", 10), kw.get("bin_ms", 1))
        assert ei.value.status == -1
    for groups, ng in (([1], 1), ([-1], 1), (None, 2)):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_trace([ok], 10, 1, groups=groups, ngroups=ng)
        assert ei.value.status == -1
    L = pkg.lib()
    sp = pkg.PrachTraceSpec(10, 1, 1, 0)
    arr, res, t = (pkg.PrachCfg * 1)(ok), (pkg.PrachResult * 1)(), (pkg.PrachTrace * 1)()
    a = [(C.c_uint64 * 10)() for _ in range(4)]
    for hole in range(5):
        outs = [t] + a
        outs[hole] = None
        assert L.prach_run_trials_trace(eng._h, arr, 1, res, None, C.byref(sp), None, *outs) == -1
    sp.reserved = 1
    assert L.prach_run_trials_trace(eng._h, arr, 1, res, None, C.byref(sp), None, t, *a) == -1
    assert L.prach_run_trials_trace(eng._h, arr, 1, res, None, None, None, t, *a) == -1


def _variant_library(name, flag):
    pkg_dir = os.path.join(ROOT, "5g-nr-randomaccess_amd")
    csrc = os.path.join(pkg_dir, "csrc")
    lib = os.path.join(pkg_dir, name)
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".c"))] + [os.path.join(ROOT, "include", "prach.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) + 1.0 for s in srcs):
        subprocess.check_call(["make", "-C", csrc, "lib", flag, "ARCH=gfx950"])
    return lib


@pytest.mark.parametrize("name,flag", [("libprach_hip_nobitop3.so", "NOBITOP3=1"), ("libprach_hip_tinyq.so", "TINYQ=1")])
def test_every_library_build(name, flag):
    """6. over_3000 through every route with the library built without v_bitop3 and with the small-queue build, each in a child process of its own."""
    lib = _variant_library(name, flag)
    # (the small-queue build exists so that ordinary trials exceed a capacity and leave their kernel: its calls are not held to a route's pin)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "gpu_trace_routes.py"), "over_3000"] + (["--no-pin"] if flag == "TINYQ=1" else []), env=dict(os.environ, PRACH_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "done" in p.stdout and " 0 bad" in p.stdout, (p.stdout[-3000:], p.stderr[-3000:])
