"""prach_run_trials_noma_timeline on the GPU: prach::noma_timeline_kernel, reducing the log records prach::noma_kernel leaves on the device, equals the host
definition integer for integer — on the ORACLE's UEs for the Philox cases of tests/test_noma_timeline_cpu.py, on the logs the same call returns for trials
around the tile size, in a 48-trial call with groups under both schemes with and without host logs, under every cluster size, under a memory budget that
splits the call and under the NOMA_AMBIGUOUS rerun (a trial counts once), and on the all-served early exit whose E comes from prach_result.steps; the timing
fields, the refusals, what a trace call and a timeline call of the same cfgs must agree on, and prach_sim --census-timeline against noma_timeline_csv."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_census_ref as N  # noqa: E402
import noma_timeline_ref as T  # noqa: E402
from test_noma_timeline_cpu import CASES, SPECS, oracle_trial, product_cfg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def noma_cfg(pkg, nUE, seed, **kw):
    return pkg.make_cfg(nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=seed, **kw)


def host_of(pkg, cfgs, res, logs, bins, bin_ms, **kw):
    return pkg.noma_timeline_from_logs(cfgs, [r.steps for r in res], logs, bins, bin_ms, **kw)


def equal(tl, host):
    assert tl.same_as(host), (T.describe(tl), T.describe(host))
    assert T.identity(tl)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "philox"], ids=lambda c: f"{c[0]}ues_seed{c[1]}")
def test_philox_cases_equal_the_host_definition_on_the_oracles_ues(pkg, ob, eng, case):
    n, seed, rng, kw = case
    c = product_cfg(pkg, n, seed, rng, kw)
    ores, a = oracle_trial(ob, n, seed, rng, kw)
    for bins, bin_ms in SPECS:
        res, logs, tl = eng.run_trials_noma_timeline([c], bins, bin_ms, want_logs=True)
        assert res[0].status == 0 and int(res[0].steps) == int(ores.steps) and np.array_equal(N.as_array(logs[0]), a)
        equal(tl, pkg.noma_timeline_from_logs([c], [ores.steps], [a], bins, bin_ms))
        sc = {f: int(v[0]) for f, v in tl.scalars.items()}
        assert sc["served"] == res[0].nSuccessUE == ores.nSuccessUE and sc["undefined"] == 0 and sc["trials"] == 1 and sc["ues"] == n
        if (bins, bin_ms) == (100, 7) and n == 2000:
            assert sc["arrival_overflow"] > 0 and sc["done_overflow"] > 0
    if kw.get("flags"):
        assert (tl.arrivals[0].sum(axis=1) > 0).all()  # PRACH_FLAG_NOMA_NONSECTOR: the UE's own sector, all six of them


def test_trials_around_the_tile_size(pkg, eng):
    tile = pkg.noma_timeline_tile_ues()
    cfgs = [noma_cfg(pkg, tile + d, 3 + d, max_steps=2500) for d in (-1, 0, 1)]
    for scheme in (0, 1):
        eng.set("timeline_scheme", scheme)
        res, logs, tl = eng.run_trials_noma_timeline(cfgs, 2002, 5, want_logs=True)
        assert all(r.status == 0 for r in res)
        equal(tl, host_of(pkg, cfgs, res, logs, 2002, 5))
        assert (tl.scalars["served"] > 0).all() and (tl.scalars["pending"] > 0).all() and (tl.scalars["idle"] > 0).all()


def small_trials(pkg, n=48):
    rng = np.random.default_rng(11)
    return [noma_cfg(pkg, int(u), k, max_steps=1200 + 100 * (k % 5) + k % 3, nGrantUL=1 + k % 3, maxMsg2TxCount=3 if k % 4 == 0 else 10, flags=2 if k % 7 == 0 else 0)
            for k, u in enumerate(rng.integers(60, 900, n))]


def test_a_48_trial_call_with_groups_both_schemes_with_and_without_logs(pkg, eng):
    cfgs = small_trials(pkg)
    groups = np.random.default_rng(5).permutation(np.arange(48) % 5).tolist()
    res, logs, per = eng.run_trials_noma_timeline(cfgs, 300, 5, want_logs=True)
    assert all(r.status == 0 for r in res)
    equal(per, host_of(pkg, cfgs, res, logs, 300, 5))
    merged = host_of(pkg, cfgs, res, logs, 300, 5, groups=groups, ngroups=7)
    assert (merged.scalars["served"][:5] > 0).all() and int(merged.scalars["pending"].sum()) > 0
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert [bytes(r) for r in res0] == [bytes(r) for r in res] and [bytes(l) for l in logs0] == [bytes(l) for l in logs]
    for scheme in (0, 1):
        eng.set("timeline_scheme", scheme)
        for want in (True, False, [3]):
            r7, l7, g7 = eng.run_trials_noma_timeline(cfgs, 300, 5, groups=groups, ngroups=7, want_logs=want)  # groups 5 and 6 have no trial
            equal(g7, merged)
            assert [bytes(r) for r in r7] == [bytes(r) for r in res]
            assert all(l is None or bytes(l) == bytes(logs[k]) for k, l in enumerate(l7)) and sum(l is not None for l in l7) == (48 if want is True else 1 if want else 0)
        assert g7.scalars["done_max"][5:].tolist() == [-1, -1] and not g7.series[:, 5:].any()
        for window in (1, 7, 1024):  # the window is a launch argument: any size gives the same integers
            eng.set("noma_timeline_window", window)
            equal(eng.run_trials_noma_timeline(cfgs, 300, 5, groups=groups, ngroups=7)[2], merged)
        eng.set("noma_timeline_window", 0)


@pytest.mark.parametrize("cluster", [1, 2, 4])
def test_cluster_sizes(pkg, eng, cluster):
    eng.set("cluster", cluster)
    cfgs = [noma_cfg(pkg, 20000, 21, max_steps=3000)]
    res, logs, tl = eng.run_trials_noma_timeline(cfgs, 2002, 5, want_logs=True)
    assert res[0].status == 0 and eng.timing().cluster_size == cluster
    equal(tl, host_of(pkg, cfgs, res, logs, 2002, 5))
    assert int(tl.scalars["served"][0]) == res[0].nSuccessUE > 0


def same_under(pkg, cfgs, *setups):
    """The same grouped call on one fresh engine per setup (None: as it is; else a function that sets options); every setup's timeline equals the first's."""
    out = []
    for fn in setups:
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            res, _, tl = e.run_trials_noma_timeline(cfgs, 600, 5, groups=[k % 2 for k in range(len(cfgs))], ngroups=2)
            assert all(r.status == 0 for r in res)
            out.append((tl, e.timing()))
        finally:
            e.close()
    for tl, _ in out[1:]:
        assert tl.same_as(out[0][0]) and int(tl.scalars["trials"].sum()) == len(cfgs) and int(tl.scalars["ues"].sum()) == sum(c.nUE for c in cfgs)
    return [t for _, t in out]


def test_counted_once_under_the_ambiguity_rerun_and_a_split_call(pkg):
    """noma_ambiguity_test = 1: every gain sort counts as ambiguous, the trials are rerun with the host-built table; mem_budget_mb = 4 splits the call.  The
    records of a discarded launch are never reduced: the timeline is the undisturbed call's, every trial counted once."""
    cfgs = [noma_cfg(pkg, 4000, s, max_steps=2500) for s in range(16)]

    def split(e):
        e.set("mem_budget_mb", 4)

    def both(e):
        e.set("noma_ambiguity_test", 1)
        e.set("mem_budget_mb", 4)

    t0, ta, ts, tb = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1), split, both)
    assert t0.fallback_trials == 0 and ta.fallback_trials >= 1 and tb.fallback_trials >= 1
    assert ta.launches > t0.launches and ts.launches > t0.launches and tb.launches > ta.launches
    assert all(t.noma_timeline_ms > 0 for t in (t0, ta, ts, tb))


def test_all_served_early_exit_takes_e_from_steps(pkg, ob, eng):
    case = (64, 14, "philox", dict(nGrantUL=30))
    c = product_cfg(pkg, *case)
    ores, a = oracle_trial(ob, *case)
    assert ores.nSuccessUE == 64 and int(ores.steps) < 10000
    res, logs, tl = eng.run_trials_noma_timeline([c], 2002, 5, want_logs=True)
    assert int(res[0].steps) == int(ores.steps) and res[0].nSuccessUE == 64
    equal(tl, pkg.noma_timeline_from_logs([c], [ores.steps], [a], 2002, 5))
    assert int(tl.scalars["served"][0]) == 64 == int(tl.done.sum()) and int(tl.scalars["pending"][0]) == 0


def test_timing_fields(pkg, eng):
    others = ("noma_trace_ms", "noma_census_ms", "noma_columns_ms", "noma_summary_ms", "noma_pick_ms", "columns_ms", "pick_ms", "xtab_ms", "trace_ms", "summary_ms", "dist_ms",
              "timeline_ms", "sojourn_ms")
    cfgs = [noma_cfg(pkg, 3000, 1, max_steps=3000)]
    eng.run_trials(cfgs)
    assert eng.timing().noma_timeline_ms == 0
    eng.run_trials_noma_timeline(cfgs, 600, 5)
    tm = eng.timing()
    assert tm.noma_timeline_ms > 0 and all(getattr(tm, f) == 0 for f in others)
    eng.run_trials_noma_trace(cfgs, 600, 5)
    tm = eng.timing()
    assert tm.noma_trace_ms > 0 and tm.noma_timeline_ms == 0
    eng.run_trials_timeline([pkg.make_cfg(3000, variant=0, rng_mode=pkg.RNG_PHILOX, seed=1)], 100, 100)
    tm = eng.timing()
    assert tm.timeline_ms > 0 and tm.noma_timeline_ms == 0


def test_refusals_leave_outputs_untouched_and_the_engine_goes_on(pkg, eng):
    L = pkg.lib()
    good = [noma_cfg(pkg, 1000, 1, max_steps=2000), noma_cfg(pkg, 500, 2, max_steps=2000)]
    for bad_cfgs in ([good[0], pkg.make_cfg(1000, variant=0, rng_mode=pkg.RNG_PHILOX)], [good[0], pkg.make_cfg(1000, variant=1, rng_mode=pkg.RNG_PHILOX)],
                     [good[0], pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]):
        n = len(bad_cfgs)
        tl = pkg.NomaTimeline(n, 400, 5)
        tl.series[:] = 7
        hdr = (pkg.PrachNomaTimeline * n)()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        sp = tl.spec()
        assert L.prach_run_trials_noma_timeline(eng._h, (pkg.PrachCfg * n)(*bad_cfgs), n, (pkg.PrachResult * n)(), None, C.byref(sp), None, hdr, tl._series()) == -2
        assert (tl.series == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)
    for bad in (dict(bins=0), dict(bins=pkg.TIMELINE_MAX_BINS + 1), dict(bins=10, bin_ms=0), dict(bins=10, ngroups=3), dict(bins=10, groups=[0, 2], ngroups=2),
                dict(bins=10, ngroups=0, groups=[0, 0])):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_timeline(good, **bad)
        assert ei.value.status == -1, bad
    sp = pkg.PrachNomaTimelineSpec(65536, 1, 64, 0)  # 36 x 64 x 65536 words > 2^27: judged before any output is touched
    one = np.zeros(1, dtype=np.uint64)
    ptrs = (C.POINTER(C.c_uint64) * 6)(*[one.ctypes.data_as(C.POINTER(C.c_uint64))] * 6)
    hdr = (pkg.PrachNomaTimeline * 64)()
    assert L.prach_run_trials_noma_timeline(eng._h, (pkg.PrachCfg * 2)(*good), 2, (pkg.PrachResult * 2)(), None, C.byref(sp), (C.c_int32 * 2)(0, 1), hdr, ptrs) == -2
    assert one[0] == 0
    with pytest.raises(pkg.PrachError) as ei:  # the other programs' timeline keeps refusing NOMA.c
        eng.run_trials_timeline(good, 100, 100)
    assert ei.value.status == -2
    res, _, tl = eng.run_trials_noma_timeline(good, 400, 5)  # the engine goes on
    assert all(r.status == 0 for r in res) and int(tl.arrivals.sum()) > 0


def test_a_trace_call_and_a_timeline_call_agree_where_they_must(pkg, eng):
    cfgs = [noma_cfg(pkg, 3000, 0), noma_cfg(pkg, 1500, 1, max_steps=4000), noma_cfg(pkg, 2000, 2, flags=2), noma_cfg(pkg, 800, 3, nGrantUL=1, maxMsg2TxCount=3)]
    groups = [0, 1, 0, 2]
    rt, _, tr = eng.run_trials_noma_trace(cfgs, 2002, 5, groups=groups, ngroups=3)
    rl, _, tl = eng.run_trials_noma_timeline(cfgs, 2002, 5, groups=groups, ngroups=3)
    assert [bytes(r) for r in rt] == [bytes(r) for r in rl]
    assert tr.series.shape == tl.series.shape  # index for index
    granted = tr.series[pkg.NOMA_TRACE_SERIES.index("granted")].astype(np.int64).sum(axis=(1, 2))
    done = tl.done.astype(np.int64).sum(axis=(1, 2))
    assert (done <= granted).all() and (done > 0).all() and (tl.scalars["done_overflow"] == 0).all()
    for g in range(3):
        assert int(tl.scalars["served"][g]) == sum(int(r.nSuccessUE) for r, k in zip(rl, groups) if k == g)
    assert int(tl.scalars["trials"].sum()) == int(tr.scalars["trials"].sum()) == 4


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_census_timeline_equals_the_binding(pkg, eng, tmp_path, workers):
    """prach_sim --program noma --census-timeline on a two-point sweep, three seeds per point merged — and the same from two forked workers on one device."""
    out = tmp_path / "timeline.csv"
    cmd = [pkg.CLI_PATH, "--program", "noma", "-t", "3", "--sweep", "1000:2000:1000", "--out", str(tmp_path), "--census-timeline", str(out)]
    bin_ms = 5
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers), "--census-timeline-bin", "50"]
        bin_ms = 50
    else:
        cmd += ["--gpus", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [1000, 2000]
    cfgs = [noma_cfg(pkg, n, s) for s in range(3) for n in points]
    _, _, exp = eng.run_trials_noma_timeline(cfgs, (10006 + bin_ms - 1) // bin_ms, bin_ms, groups=[k % 2 for k in range(6)], ngroups=2)
    assert out.read_bytes() == pkg.noma_timeline_csv(exp, labels=points) and len(out.read_bytes()) > 300
    assert int(exp.scalars["arrival_overflow"].sum()) == int(exp.scalars["done_overflow"].sum()) == 0  # the bins cover 10 000 + 6 subframes
