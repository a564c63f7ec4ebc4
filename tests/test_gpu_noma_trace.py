"""prach_run_trials_noma_trace on the GPU: the rows prach::noma_kernel records while it runs, reduced by prach::noma_trace_kernel, equal the exact CPU reference
built from the oracle alone (tests/tools/noma_trace_ref.py, tests/tools/NOMA_TRACE.md) — singles, granted, pairs and pair_one at every slot, tx and used at a
spread subset of the slots (every slot on the smallest case) — on the trial cases of noma_trace_ref.CASES, under every cluster size, in a 48-trial call with
groups, with and without host logs, under both schemes, under a memory budget that splits the call and under the NOMA_AMBIGUOUS rerun (a trial counts once);
coarser and non-dividing bins equal a numpy re-binning; results and logs are those of plain prach_run_trials; the refusals hold; prach_sim --census-trace
writes noma_trace_csv byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_trace_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def noma_cfg(pkg, nUE, seed, **kw):
    return pkg.make_cfg(nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=seed, **kw)


def case_cfg(pkg, case):
    k = dict(R.CASES[case])
    return noma_cfg(pkg, k.pop("nUE"), k.pop("seed"), **k)


def device_rows(tr, g, slots):
    """Group g of a trace taken at bin_ms = accessTime as rows [slots, 6 sectors, 6 series]; nothing lies behind them."""
    s = tr.series[:, g].astype(np.int64)  # [6 series, 6 sectors, bins]
    assert not s[:, :, slots:].any()
    return np.ascontiguousarray(s[:, :, :slots].transpose(2, 1, 0))


def equals_reference(dev, rows, mask):
    assert dev.shape == rows.shape, (dev.shape, rows.shape)
    assert np.array_equal(dev[..., R.SINGLES:], rows[..., R.SINGLES:])           # every slot
    assert np.array_equal(dev[mask][..., :R.SINGLES], rows[mask][..., :R.SINGLES])  # tx, used: where the stopped runs were made
    assert mask.sum() >= 8 or mask.all()


def scalars_of_rows(tr, g, dev):
    sc = tr.scalars
    assert [int(sc[f][g]) for f in R.SERIES] == dev.sum(axis=(0, 1)).tolist() and int(sc["slots"][g]) == len(dev) and int(sc["overflow_tx"][g]) == 0
    assert int(sc["tx_max"][g]) == (int(dev[..., R.TX].max()) if len(dev) else -1) and int(sc["trials"][g]) == 1


def traced(pkg, eng, cfgs, want_logs=True, **kw):
    """One call at bin_ms = accessTime (one accessTime per call) with bins for the longest trial; plain results and logs are those of prach_run_trials."""
    aT = cfgs[0].accessTime
    assert all(c.accessTime == aT for c in cfgs)
    bins = max((int(pkg.lib().prach_max_time(C.byref(c))) + aT - 1) // aT for c in cfgs)
    res, logs, tr = eng.run_trials_noma_trace(cfgs, bins, aT, want_logs=want_logs, **kw)
    assert all(r.status == 0 for r in res)
    return res, logs, tr


@pytest.mark.parametrize("case", [c for c in R.CASES if c != "cluster"])
def test_trial_cases_equal_the_oracle(pkg, ob, eng, case):
    c = case_cfg(pkg, case)
    oc, ores, rows, mask, oues = R.case_trial(ob, case)
    assert bytes(R.oracle_cfg(ob, c)) == bytes(oc)  # the case in the library's terms is the case in the oracle's
    R.check_identities(rows, mask, oc.nGrantUL, oc.nPreamble)
    assert int(rows[..., R.GRANTED].sum()) == R.grants_of_ues(oues)
    res, logs, tr = traced(pkg, eng, [c])
    assert int(res[0].steps) == int(ores.steps) and len(rows) == R.nslots(res[0].steps, c.accessTime)
    dev = device_rows(tr, 0, len(rows))
    equals_reference(dev, rows, mask)
    scalars_of_rows(tr, 0, dev)
    R.check_identities(dev, np.ones(len(dev), dtype=bool), c.nGrantUL, c.nPreamble)  # on the device's rows tx and used are known everywhere
    assert int(dev[..., R.GRANTED].sum()) == R.grants_of_ues(R.as_array(logs[0])) == R.grants_of_ues(oues)  # on the logs the same call returns
    res0, logs0 = eng.run_trials([c], want_logs=True)
    assert bytes(res0[0]) == bytes(res[0]) and bytes(logs0[0]) == bytes(logs[0])
    if case == "cellwide":
        assert not dev[:, 1:].any() and int((dev[..., R.USED] - dev[..., R.SINGLES]).sum()) > 0
    if case == "all_states_partial":
        assert c.max_steps % c.accessTime != 0 and dev[-1].any() == rows[-1].any()
    if case == "last_preamble":
        assert c.nPreamble == 64 and c.accessTime == 10
    if case == "early_exit":
        assert res[0].nSuccessUE == c.nUE and int(res[0].steps) < 10000 and mask.all()
    if case == "full_run":
        assert len(dev) == 2000


@pytest.mark.parametrize("cluster", [1, 4, 32])
def test_cluster_sizes_write_cluster_totals_once(pkg, ob, eng, cluster):
    eng.set("cluster", cluster)
    c = case_cfg(pkg, "cluster")
    oc, ores, rows, mask, oues = R.case_trial(ob, "cluster")
    assert int(rows[..., R.SINGLES].max()) == 11 and int(rows[..., R.PAIRS].sum()) == 1009
    res, logs, tr = traced(pkg, eng, [c])
    assert eng.timing().cluster_size == cluster
    dev = device_rows(tr, 0, len(rows))
    equals_reference(dev, rows, mask)
    scalars_of_rows(tr, 0, dev)
    R.check_identities(dev, np.ones(len(dev), dtype=bool), c.nGrantUL, c.nPreamble)
    assert int(dev[..., R.GRANTED].sum()) == R.grants_of_ues(R.as_array(logs[0])) == 4187


def small_trials(pkg, n=48):
    rng = np.random.default_rng(11)
    return [noma_cfg(pkg, int(u), k, max_steps=1200 + 100 * (k % 5) + k % 3, nGrantUL=1 + k % 3, flags=2 if k % 7 == 0 else 0) for k, u in enumerate(rng.integers(60, 900, n))]


def test_a_48_trial_call_with_groups_both_schemes_with_and_without_logs(pkg, ob, eng):
    cfgs = small_trials(pkg)
    groups = np.random.default_rng(5).permutation(np.arange(48) % 5).tolist()
    res, logs, per = traced(pkg, eng, cfgs)
    for k, c in enumerate(cfgs):  # singles, granted, pairs, pair_one of every trial against the sector hook; sum(granted) against the logs
        ores, rows = R.resolved(ob, R.oracle_cfg(ob, c), c.seed)
        dev = device_rows(per, k, len(rows))
        assert np.array_equal(dev[..., R.SINGLES:], rows[..., R.SINGLES:]), k
        assert int(dev[..., R.GRANTED].sum()) == R.grants_of_ues(R.as_array(logs[k]))
        R.check_identities(dev, np.ones(len(dev), dtype=bool), c.nGrantUL, c.nPreamble)
    assert int(per.series[R.PAIRS].sum()) > 0 and int(per.scalars["trials"].sum()) == 48
    merged = pkg.NomaTrace(7, per.bins, per.bin_ms)
    for k, g in enumerate(groups):
        merged.merge_group(g, per, k)
    for scheme in (0, 1):
        eng.set("trace_scheme", scheme)
        for want in (True, False, [3]):
            r7, l7, g7 = eng.run_trials_noma_trace(cfgs, per.bins, per.bin_ms, groups=groups, ngroups=7, want_logs=want)  # groups 5 and 6 have no trial
            assert g7.same_as(merged) and [bytes(r) for r in r7] == [bytes(r) for r in res]
            assert all(l is None or bytes(l) == bytes(logs[k]) for k, l in enumerate(l7)) and sum(l is not None for l in l7) == (48 if want is True else 1 if want else 0)
        assert g7.scalars["tx_max"][5:].tolist() == [-1, -1] and not g7.series[:, 5:].any()
        _, _, p0 = traced(pkg, eng, cfgs, want_logs=False)
        assert p0.same_as(per)


def test_coarser_and_non_dividing_bins_equal_a_numpy_rebinning(pkg, eng):
    cfgs = [case_cfg(pkg, "all_states"), case_cfg(pkg, "cellwide"), noma_cfg(pkg, 3000, 2, max_steps=3001)]
    res, _, fine = traced(pkg, eng, cfgs, want_logs=False)
    rows = [device_rows(fine, k, R.nslots(r.steps, 5)) for k, r in enumerate(res)]
    for scheme in (0, 1):
        eng.set("trace_scheme", scheme)
        for bins, bin_ms, groups, ng in ((2000, 5, None, None), (400, 25, None, None), (77, 13, [1, 0, 1], 2), (5000, 2, None, None), (65536, 1, [0, 0, 0], 1), (40, 100, [2, 2, 0], 4),
                                         (1, 10000, None, None), (1, 1, None, None), (150, 7, [0, 1, 0], 2)):
            _, _, tr = eng.run_trials_noma_trace(cfgs, bins, bin_ms, groups=groups, ngroups=ng)
            series, sc = R.rebin(rows, [5, 5, 5], bins, bin_ms, groups, tr.ngroups)
            assert R.same(tr, series, sc), (scheme, bins, bin_ms)
            assert (int(sc["overflow_tx"].sum()) > 0) == (bins * bin_ms < 5000)  # (the longest of the three runs 5000 subframes)


def same_under(pkg, cfgs, *setups):
    """The same grouped call on one fresh engine per setup (None: as it is; else a function that sets options); every setup's trace equals the first's."""
    out = []
    for fn in setups:
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            res, _, tr = e.run_trials_noma_trace(cfgs, 600, 5, groups=[k % 2 for k in range(len(cfgs))], ngroups=2)
            assert all(r.status == 0 for r in res)
            out.append((tr, e.timing()))
        finally:
            e.close()
    for tr, _ in out[1:]:
        assert tr.same_as(out[0][0]) and int(tr.scalars["trials"].sum()) == len(cfgs)
    return [t for _, t in out]


def test_counted_once_under_the_ambiguity_rerun_and_a_split_call(pkg):
    """noma_ambiguity_test = 1 (devact == 2): every gain sort counts as ambiguous, the trials are rerun with the host-built table; mem_budget_mb = 4 splits the
    call on the layout that holds the rows.  The rows of a discarded launch are never read: the trace is the undisturbed call's, every trial counted once."""
    cfgs = [noma_cfg(pkg, 4000, s, max_steps=2500) for s in range(16)]

    def split(e):
        e.set("mem_budget_mb", 4)

    def both(e):
        e.set("noma_ambiguity_test", 1)
        e.set("mem_budget_mb", 4)

    t0, ta, ts, tb = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1), split, both)
    assert t0.fallback_trials == 0 and ta.fallback_trials >= 1 and tb.fallback_trials >= 1
    assert ta.launches > t0.launches and ts.launches > t0.launches and tb.launches > ta.launches
    assert all(t.noma_trace_ms > 0 for t in (t0, ta, ts, tb))


def test_timing_fields(pkg, eng):
    others = ("noma_census_ms", "noma_columns_ms", "noma_summary_ms", "noma_pick_ms", "columns_ms", "pick_ms", "xtab_ms", "trace_ms", "summary_ms", "dist_ms", "timeline_ms", "sojourn_ms")
    cfgs = [noma_cfg(pkg, 3000, 1, max_steps=3000)]
    eng.run_trials(cfgs)
    assert eng.timing().noma_trace_ms == 0
    eng.run_trials_noma_trace(cfgs, 600, 5)
    tm = eng.timing()
    assert tm.noma_trace_ms > 0 and all(getattr(tm, f) == 0 for f in others)
    eng.run_trials_noma_census(cfgs)
    tm = eng.timing()
    assert tm.noma_census_ms > 0 and tm.noma_trace_ms == 0
    eng.run_trials_trace([pkg.make_cfg(3000, variant=0, rng_mode=pkg.RNG_PHILOX, seed=1)], 100, 100)
    tm = eng.timing()
    assert tm.trace_ms > 0 and tm.noma_trace_ms == 0


def test_refusals_leave_outputs_untouched_and_the_engine_goes_on(pkg, eng):
    L = pkg.lib()
    good = [noma_cfg(pkg, 1000, 1, max_steps=2000), noma_cfg(pkg, 500, 2, max_steps=2000)]
    for bad_cfgs in ([good[0], pkg.make_cfg(1000, variant=0, rng_mode=pkg.RNG_PHILOX)], [good[0], pkg.make_cfg(1000, variant=1, rng_mode=pkg.RNG_PHILOX)],
                     [good[0], pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]):
        n = len(bad_cfgs)
        arr = (pkg.PrachCfg * n)(*bad_cfgs)
        res = (pkg.PrachResult * n)()
        tr = pkg.NomaTrace(n, 400, 5)
        tr.series[:] = 7
        hdr = (pkg.PrachNomaTrace * n)()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        sp = tr.spec()
        assert L.prach_run_trials_noma_trace(eng._h, arr, n, res, None, C.byref(sp), None, hdr, tr._series()) == -2
        assert (tr.series == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)
    for bad in (dict(bins=0), dict(bins=pkg.TRACE_MAX_BINS + 1), dict(bins=10, bin_ms=0), dict(bins=10, ngroups=3), dict(bins=10, groups=[0, 2], ngroups=2), dict(bins=10, ngroups=0, groups=[0, 0])):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_trace(good, **bad)
        assert ei.value.status == -1, bad
    sp = pkg.PrachNomaTraceSpec(65536, 1, 64, 0)  # 36 x 64 x 65536 words > 2^27: judged before any output is touched
    n = 2
    arr = (pkg.PrachCfg * n)(*good)
    res = (pkg.PrachResult * n)()
    one = np.zeros(1, dtype=np.uint64)
    ptrs = (C.POINTER(C.c_uint64) * 6)(*[one.ctypes.data_as(C.POINTER(C.c_uint64))] * 6)
    hdr = (pkg.PrachNomaTrace * 64)()
    assert L.prach_run_trials_noma_trace(eng._h, arr, n, res, None, C.byref(sp), (C.c_int32 * 2)(0, 1), hdr, ptrs) == -2
    with pytest.raises(pkg.PrachError) as ei:  # the per-subframe trace keeps refusing NOMA.c
        eng.run_trials_trace(good, 100, 100)
    assert ei.value.status == -2
    res, _, tr = eng.run_trials_noma_trace(good, 400, 5)  # the engine goes on
    assert all(r.status == 0 for r in res) and int(tr.scalars["tx"].sum()) > 0


def test_ratios(pkg, eng):
    c = case_cfg(pkg, "cellwide")
    _, _, tr = eng.run_trials_noma_trace([c], 50, 100)
    s = tr.series[:, 0].sum(axis=1).astype(np.float64)
    cr, ns = tr.collision_ratio(0), tr.noma_share(0)
    assert np.array_equal(np.isnan(cr), s[R.USED] == 0) and np.array_equal(np.isnan(ns), s[R.GRANTED] == 0)
    ok = s[R.USED] > 0
    assert np.array_equal(cr[ok], (s[R.USED][ok] - s[R.SINGLES][ok]) / s[R.USED][ok]) and (cr[ok] > 0).any()
    ok = s[R.GRANTED] > 0
    assert np.array_equal(ns[ok], (2 * s[R.PAIRS][ok] - s[R.PAIR_ONE][ok]) / s[R.GRANTED][ok]) and (ns[ok] > 0).any() and (ns[ok] <= 1).all()


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_census_trace_equals_the_binding(pkg, eng, tmp_path, workers):
    """prach_sim --program noma --census-trace on a two-point sweep, three seeds per point merged — and the same from two forked workers on one device."""
    out = tmp_path / "trace.csv"
    cmd = [pkg.CLI_PATH, "--program", "noma", "-t", "3", "--sweep", "1000:2000:1000", "--out", str(tmp_path), "--census-trace", str(out)]
    bin_ms = 5
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers), "--census-trace-bin", "50"]
        bin_ms = 50
    else:
        cmd += ["--gpus", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [1000, 2000]
    cfgs = [noma_cfg(pkg, n, s) for s in range(3) for n in points]
    _, _, exp = eng.run_trials_noma_trace(cfgs, (10000 + bin_ms - 1) // bin_ms, bin_ms, groups=[k % 2 for k in range(6)], ngroups=2)
    assert out.read_bytes() == pkg.noma_trace_csv(exp, labels=points) and len(out.read_bytes()) > 300
    for extra, msg in ((["--rng", "glibc"], "--census-trace"), (["--census", str(tmp_path / "c.csv")], "one reduction per call")):
        p = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and msg in p.stdout, (extra, p.stdout[-300:])  # (prach_sim's refusals go to its standard output)
    p = subprocess.run([pkg.CLI_PATH, "--program", "beta", "--census-trace", str(out)], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--census-trace needs --program noma" in p.stdout
