"""prach_run_trials_summary on the GPU: the per-trial rows prach::summary_kernel selects on the device equal, integer for integer, prach_summary_from_logs of
the per-UE logs the same call returns, a numpy restatement (np.sort, the integer rank rule) over those logs and over the oracle's UEs: in both RNG modes,
behind every kernel, under the reruns the engine knows (a row is written once), with and without host logs, and through prach_sim --ci and sweep.py --ci."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import summary_ref as R  # noqa: E402
import timeline_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = (1, 250, 500, 501, 900, 950, 990, 1000)


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def refs(pkg, cfgs, arrays, levels):
    return [R.trial_row(a, pkg.arrival_schedule(c)[0], c.accessTime, levels) for c, a in zip(cfgs, arrays)]


def run_checked(pkg, eng, cfgs, levels=LEVELS):
    """One call with logs: the device's rows equal summary_from_logs and numpy on the logs of the same call."""
    res, logs, sm = eng.run_trials_summary(cfgs, levels, want_logs=True)
    assert all(r.status == 0 for r in res)
    host = pkg.summary_from_logs(cfgs, logs, levels)
    want = refs(pkg, cfgs, [T.as_array(l) for l in logs], levels)
    R.check_rows(host.rows, want)
    R.check_rows(sm.rows, want)
    assert sm.rows["nUE"].tolist() == [c.nUE for c in cfgs] and sm.rows["success"].tolist() == [r.nSuccessUE for r in res]
    assert sm.rows["arrived"].tolist() == [r.activeCheck for r in res] and sm.rows["timer_sum"].tolist() == [r.sumTimer for r in res]
    tm = eng.timing()
    assert tm.summary_ms > 0 and tm.dist_ms == 0 and tm.timeline_ms == 0 and tm.sojourn_ms == 0
    return res, logs, sm


_oracle = {}


def oracle_array(ob, c):
    key = bytes(c)
    if key not in _oracle:
        res, ues = ob.run_trial(T.oracle_cfg(ob, c), ob.Rng(c.rng_mode, c.seed))
        _oracle[key] = T.as_array(ues).copy()
    return _oracle[key]


def trial_cfgs(pkg, rng_mode):
    """nUE <= 3000: Beta.c and RandomAccessWithNOMA, one with restarts, Uniform traffic, a trial cut after 3 subframes (nobody succeeds), odd sizes."""
    return [pkg.make_cfg(3000, variant=0, rng_mode=rng_mode, seed=1), pkg.make_cfg(2000, variant=1, rng_mode=rng_mode, seed=2, maxMsg2TxCount=3),
            pkg.make_cfg(500, variant=0, rng_mode=rng_mode, seed=3, uniform=1), pkg.make_cfg(300, variant=0, rng_mode=rng_mode, seed=4, max_steps=3),
            pkg.make_cfg(1, variant=1, rng_mode=rng_mode, seed=5), pkg.make_cfg(65, variant=0, rng_mode=rng_mode, seed=6), pkg.make_cfg(1025, variant=1, rng_mode=rng_mode, seed=7)]


# the batch kernels (the default of a one-workgroup-per-trial call); trial_kernel; the general cluster kernel with one workgroup per trial (the engine has no
# "batch" switch: 16-byte records keep a call off the batch kernel, as in tests/tools/kernel_matrix.py); lean clusters of 4; general clusters of 4; and the
# summary kernel's other workgroup shape
KERNELS = {"default": {}, "legacy": dict(legacy=1), "no_batch": dict(cluster=1, wide_records=1), "cluster4": dict(cluster=4), "cluster4_no_fast": dict(cluster=4, fast=0),
           "threads512": dict(summary_threads=512)}


@pytest.mark.parametrize("rng", ["glibc", "philox"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_rows_equal_logs_numpy_and_oracle(pkg, ob, eng, kernel, rng):
    for k, v in KERNELS[kernel].items():
        eng.set(k, v)
    cfgs = trial_cfgs(pkg, pkg.RNG_GLIBC if rng == "glibc" else pkg.RNG_PHILOX)
    res, logs, sm = run_checked(pkg, eng, cfgs)
    R.check_rows(sm.rows, refs(pkg, cfgs, [oracle_array(ob, c) for c in cfgs], LEVELS))
    assert int(sm.rows[1]["restarted"]) > 0 and int(sm.rows[3]["success"]) == 0 and (sm.rows[3]["q"] == -1).all() and int(sm.rows[3]["sojourn_max"]) == -1
    assert (sm.rows["q"][[0, 1, 2], :, :] >= 0).all()


def test_with_and_without_logs_and_next_to_plain_run_trials(pkg, eng):
    cfgs = trial_cfgs(pkg, pkg.RNG_PHILOX)
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().summary_ms == 0
    res1, logs1, sm1 = run_checked(pkg, eng, cfgs, (500, 950, 990))
    res2, nologs, sm2 = eng.run_trials_summary(cfgs)  # the default levels, no host logs
    assert nologs == [None] * len(cfgs) and eng.timing().summary_ms > 0
    res3, some, sm3 = eng.run_trials_summary(cfgs, (500, 950, 990), want_logs=[1])
    assert some[0] is None and bytes(some[1]) == bytes(logs0[1])
    for sm in (sm2, sm3):
        assert sm.permille == (500, 950, 990) and all(np.array_equal(sm.rows[f], sm1.rows[f]) for f in sm1.rows.dtype.names)
    for res in (res1, res2, res3):
        assert [bytes(r) for r in res] == [bytes(r) for r in res0]
    assert all(bytes(a) == bytes(b) for a, b in zip(logs1, logs0))
    eng.run_trials(cfgs)
    tm = eng.timing()
    assert tm.summary_ms == 0 and tm.dist_ms == 0 and tm.timeline_ms == 0 and tm.sojourn_ms == 0
    _, _, tl = eng.run_trials_timeline(cfgs, 16, 5000)  # the reductions share one device buffer: a summary after a timeline, and the timeline's own scalars
    _, _, sm4 = eng.run_trials_summary(cfgs, (500, 950, 990))
    assert all(np.array_equal(sm4.rows[f], sm1.rows[f]) for f in sm1.rows.dtype.names)
    for f in ("arrived", "success", "restarted", "sojourn_sum", "timer_sum"):
        assert sm4.rows[f].tolist() == tl.scalars[f].tolist()
    st = sm1.stats()  # statistics over the trials of the call, from the C function
    assert int(st[0, 0]["n"]) == len(cfgs) and int(st[0, 1]["n"]) == int((sm1.rows["success"] > 0).sum()) < len(cfgs) and float(st[0, 0]["min"]) == 0.0


def test_refusals(pkg, eng):
    cfgs = trial_cfgs(pkg, pkg.RNG_PHILOX)[:2]
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c: refused before anything is launched
        eng.run_trials_summary(cfgs + [pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1)])
    assert ei.value.status == -2
    for levels in ((), (0,), (500, 1001), tuple(range(1, 10))):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_summary(cfgs, levels)
        assert ei.value.status == -1
    with pytest.raises(pkg.PrachError):
        eng.set("summary_threads", 256)


def undisturbed_then(pkg, cfgs, disturb):
    """The rows of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, sm = run_checked(pkg, e, cfgs, (500, 950, 990))
            out.append((sm, e.timing()))
        finally:
            e.close()
    (a, t0), (b, t1) = out
    assert all(np.array_equal(a.rows[f], b.rows[f]) for f in a.rows.dtype.names)
    return t0, t1


def test_written_once_calendar_rerun(pkg):
    cases = [(3000, {}), (8000, dict(nGrantUL=3)), (12000, dict(nGrantUL=2))]  # the shapes of test_calendar_cap_rerun_is_exact: lists of 64 entries fill
    cfgs = [pkg.make_cfg(n, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s, **kw) for s in (0, 1) for n, kw in cases]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("calendar_cap", 64))
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1.launches > t0.launches


def test_written_once_mem_budget_split(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(8) for v in (0, 1) for n in (3000, 6000)]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("mem_budget_mb", 64))
    assert t1.launches >= 2 and t1.launches > t0.launches


POINTS = [1000, 2000, 3000]


def expected_csv(pkg, eng, levels):
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in POINTS]
    _, _, sm = eng.run_trials_summary(cfgs, levels)
    text = pkg.summary_csv(sm, groups=[k % 3 for k in range(9)], ngroups=3, labels=POINTS)
    assert len(text.splitlines()) == 3 * (5 + 3 * len(levels)) and text.startswith(b"1000,success_ratio,3,")
    return text


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_ci_equals_summary_csv(pkg, eng, tmp_path, workers):
    """prach_sim --ci with --logs 0 on a 3-seed x 3-point sweep — and the same from two forked workers on one device: the rows go through the shared mapping."""
    out = tmp_path / "ci.csv"
    cmd = [pkg.CLI_PATH, "--program", "beta", "-t", "3", "--rng", "philox", "--logs", "0", "--sweep", "1000:3000:1000", "--out", str(tmp_path), "--ci", str(out)]
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers), "--ci-levels", "500,999"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    assert out.read_bytes() == expected_csv(pkg, eng, (500, 999) if workers > 1 else (500, 950, 990))
    if workers == 1:
        bad = subprocess.run(cmd + ["--sojourn", str(out)], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--ci cannot be combined" in bad.stdout


def test_sweep_driver_ci_two_ranks(pkg, eng, tmp_path):
    """sweep.py --ci with 2 ranks rehearsed on one GPU (gloo): the rows are gathered to rank 0, which writes the statistics of the rows in trial order."""
    out = tmp_path / "ci.csv"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29543",
           os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--times", "3", "--sweep", "1000:3000:1000", "--out", str(tmp_path), "--backend", "gloo",
           "--same-device", "--ci", str(out), "--ci-levels", "500,950,990"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_bytes() == expected_csv(pkg, eng, (500, 950, 990))
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--ci", str(out), "--timeline", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--ci cannot be combined" in bad.stderr
