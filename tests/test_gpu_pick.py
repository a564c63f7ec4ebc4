"""prach_run_trials_pick on the GPU: the headers and rows prach::pick_kernel selects on the device (sorted by the engine) equal, integer for integer,
prach_pick_from_logs of the per-UE logs the same call returns, a numpy restatement (np.lexsort on key and index) over those logs and over the oracle's UEs:
in both RNG modes, behind every kernel, under the reruns the engine knows (a trial is written once), with and without host logs, with ties cut at the
threshold, and through prach_sim --pick and sweep.py --pick."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import pick_ref as P  # noqa: E402
import timeline_ref as T  # noqa: E402
import xtab_ref as X  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = X.SERVED | X.UNSERVED | X.IDLE
# (where, order, key, k, who): by index, both key orders, clauses with and without a(i), STATE and PTC (the record words read only then), k beyond the matches
SPECS = [((), "index", None, 16, ALL), ((), "largest", "sojourn", 16, X.SERVED), ((("state", 1, 3), ("arrival", 1000, 6000)), "smallest", "timer", 7, ALL),
         ((), "largest", "ptc", 8, X.SERVED | X.UNSERVED), ((("age", 0, 70000),), "largest", "failcount", 4096, ALL), ((("completion", 0, 4000),), "smallest", "arrival", 33, X.SERVED)]


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def refs(pkg, cfgs, arrays, ends, pk):
    return [P.numpy_pick(a, pkg.arrival_schedule(c)[0], c.accessTime, E, pk.where, pk.order, pk.key, pk.k, pk.who) for c, a, E in zip(cfgs, arrays, ends)]


def run_checked(pkg, eng, cfgs, spec):
    """One call with logs: the device's headers and rows equal pick_from_logs and numpy on the logs of the same call."""
    res, logs, pk = eng.run_trials_pick(cfgs, *spec, want_logs=True)
    assert all(r.status == 0 for r in res)
    host = pkg.pick_from_logs(cfgs, [r.steps for r in res], logs, *spec)
    want = refs(pkg, cfgs, [T.as_array(l) for l in logs], [min(r.steps, r.maxTime) for r in res], pk)
    P.check(host, want)
    P.check(pk, want)
    assert pk.same_as(host) and pk.headers["nUE"].tolist() == [c.nUE for c in cfgs] and not pk.headers["range_errors"].any()
    tm = eng.timing()
    assert tm.pick_ms > 0 and (tm.xtab_ms, tm.trace_ms, tm.summary_ms, tm.dist_ms, tm.timeline_ms, tm.sojourn_ms) == (0, 0, 0, 0, 0, 0)
    return res, logs, pk


_oracle = {}


def oracle_trial(ob, c):
    """(the oracle's UEs, its E) of a config, computed once."""
    key = bytes(c)
    if key not in _oracle:
        res, ues = ob.run_trial(T.oracle_cfg(ob, c), ob.Rng(c.rng_mode, c.seed))
        _oracle[key] = (T.as_array(ues).copy(), min(res.steps, res.maxTime))
    return _oracle[key]


def trial_cfgs(pkg, rng_mode):
    """nUE <= 3000: Beta.c and RandomAccessWithNOMA, one with restarts, Uniform traffic, a trial cut after 3 subframes (idle UEs, nobody served), odd sizes."""
    return [pkg.make_cfg(3000, variant=0, rng_mode=rng_mode, seed=1), pkg.make_cfg(2000, variant=1, rng_mode=rng_mode, seed=2, maxMsg2TxCount=3),
            pkg.make_cfg(500, variant=0, rng_mode=rng_mode, seed=3, uniform=1), pkg.make_cfg(300, variant=0, rng_mode=rng_mode, seed=4, max_steps=3),
            pkg.make_cfg(1, variant=1, rng_mode=rng_mode, seed=5), pkg.make_cfg(65, variant=0, rng_mode=rng_mode, seed=6), pkg.make_cfg(1025, variant=1, rng_mode=rng_mode, seed=7)]


# the simulation kernels as tests/test_gpu_summary.py selects them, and the pick kernel's other workgroup shape
KERNELS = {"default": {}, "legacy": dict(legacy=1), "no_batch": dict(cluster=1, wide_records=1), "cluster4": dict(cluster=4), "cluster4_no_fast": dict(cluster=4, fast=0),
           "threads512": dict(pick_threads=512)}


@pytest.mark.parametrize("rng", ["glibc", "philox"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_picks_equal_logs_numpy_and_oracle(pkg, ob, eng, kernel, rng):
    for k, v in KERNELS[kernel].items():
        eng.set(k, v)
    cfgs = trial_cfgs(pkg, pkg.RNG_GLIBC if rng == "glibc" else pkg.RNG_PHILOX)
    oracle = [oracle_trial(ob, c) for c in cfgs]
    for spec in SPECS:
        res, logs, pk = run_checked(pkg, eng, cfgs, spec)
        P.check(pk, refs(pkg, cfgs, [a for a, _ in oracle], [E for _, E in oracle], pk))
    assert int(pk.headers["matched"][3]) == 0 and int(pk.headers["stored"][0]) == 33  # (the last spec: nobody is served in the cut trial)


def test_ties_are_cut_at_the_threshold(pkg, ob, eng):
    """The overloaded 20 000-UE trial (2218 UEs left in the system): more UEs share the k-th largest preamble count, and the k-th largest failCount, than
    there are slots left; the first ones by index are kept.  The condition is asserted on the oracle's UEs."""
    c = pkg.make_cfg(20000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=7, maxMsg2TxCount=3, nPreamble=54, backoff=20, maxRarWindow=6, accessTime=5, nGrantUL=12)
    a, E = oracle_trial(ob, c)
    for spec in (((), "largest", "ptc", 8, X.UNSERVED), ((("state", 2, 5),), "largest", "failcount", 40, ALL), ((), "smallest", "timer", 7, X.UNSERVED)):
        for threads in (1024, 512):
            eng.set("pick_threads", threads)
            res, logs, pk = run_checked(pkg, eng, [c], spec)
            (hdr, rows), = refs(pkg, [c], [a], [E], pk)
            assert hdr["ties_left_out"] > 0 and hdr["matched"] == 2218 and hdr["stored"] == pk.k  # on the oracle's UEs
            P.check(pk, [(hdr, rows)])
            assert int(pk.headers["threshold"][0]) == int(pk.rows["key"][0, pk.k - 1]) == hdr["threshold"]


def test_with_and_without_logs_and_next_to_plain_run_trials(pkg, eng):
    cfgs = trial_cfgs(pkg, pkg.RNG_PHILOX)
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().pick_ms == 0
    res1, logs1, pk1 = run_checked(pkg, eng, cfgs, SPECS[1])
    res2, nologs, pk2 = eng.run_trials_pick(cfgs, *SPECS[1])  # no host logs
    assert nologs == [None] * len(cfgs) and eng.timing().pick_ms > 0
    res3, some, pk3 = eng.run_trials_pick(cfgs, *SPECS[1], want_logs=[1])
    assert some[0] is None and bytes(some[1]) == bytes(logs0[1])
    assert pk2.same_as(pk1) and pk3.same_as(pk1)
    for res in (res1, res2, res3):
        assert [bytes(r) for r in res] == [bytes(r) for r in res0]
    assert all(bytes(a) == bytes(b) for a, b in zip(logs1, logs0))
    eng.run_trials(cfgs)
    assert eng.timing().pick_ms == 0
    _, _, xt = eng.run_trials_xtab(cfgs)  # the reductions share one device buffer: a pick after a cross-tabulation, and a cell of it as a predicate
    assert eng.timing().pick_ms == 0 and eng.timing().xtab_ms > 0
    _, _, pk4 = eng.run_trials_pick(cfgs, *SPECS[1])
    assert pk4.same_as(pk1)
    r, q = np.unravel_index(int(np.argmax(xt.cells[0])), xt.cells[0].shape)
    _, _, cell = eng.run_trials_pick(cfgs, xt.cell_clauses(r, q), k=4)
    assert cell.headers["matched"].tolist() == xt.cells[:, r, q].tolist() and int(cell.headers["matched"][0]) > 4 == int(cell.headers["stored"][0])


def test_refusals(pkg, eng):
    cfgs = trial_cfgs(pkg, pkg.RNG_PHILOX)[:2]
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c: refused before anything is launched
        eng.run_trials_pick(cfgs + [pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1)])
    assert ei.value.status == -2
    for kw in (dict(k=0), dict(k=4097), dict(where=(("state", 3, 2),)), dict(where=(("one", 0, 0),) * 5), dict(who=0), dict(order=3), dict(key="timer"), dict(order="largest", key=9)):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_pick(cfgs, **kw)
        assert ei.value.status == -1, kw
    with pytest.raises(pkg.PrachError):
        eng.set("pick_threads", 256)
    res, _, pk = eng.run_trials_pick(cfgs)  # ... and the engine goes on
    assert all(r.status == 0 for r in res) and pk.headers["stored"].tolist() == [16, 16]


def undisturbed_then(pkg, cfgs, disturb, spec):
    """The picks of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, pk = run_checked(pkg, e, cfgs, spec)
            out.append((pk, e.timing()))
        finally:
            e.close()
    (a, t0), (b, t1) = out
    assert a.same_as(b)
    return t0, t1


def test_written_once_calendar_rerun(pkg):
    cases = [(3000, {}), (8000, dict(nGrantUL=3)), (12000, dict(nGrantUL=2))]  # the shapes of test_calendar_cap_rerun_is_exact: lists of 64 entries fill
    cfgs = [pkg.make_cfg(n, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s, **kw) for s in (0, 1) for n, kw in cases]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("calendar_cap", 64), SPECS[3])
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1.launches > t0.launches


def test_written_once_mem_budget_split(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(8) for v in (0, 1) for n in (3000, 6000)]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("mem_budget_mb", 64), SPECS[2])
    assert t1.launches >= 2 and t1.launches > t0.launches


POINTS = [1000, 2000, 3000]
CLI_SPEC = ((("state", 1, 1), ("ptc", 2, 200)), "largest", "sojourn", 5, X.SERVED | X.UNSERVED)
CLI_ARGS = ["--pick-where", "state:1:1", "--pick-where", "ptc:2:200", "--pick-top", "sojourn", "--pick-k", "5", "--pick-who", "arrived"]


def expected_csv(pkg, eng, spec=CLI_SPEC):
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in POINTS]
    _, _, pk = eng.run_trials_pick(cfgs, *spec)
    text = pkg.pick_csv(pk, cfgs)
    assert len(text.splitlines()) == 9 * (1 + spec[3]) and text.startswith(b"1000,0,0,1000,header,0,") and b"\n3000,8,2,3000,header,0," in text
    return text


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_pick_equals_pick_csv(pkg, eng, tmp_path, workers):
    """prach_sim --pick with --logs 0 on a 3-seed x 3-point sweep — and the same from two forked workers on one device: the rows go through the shared mapping."""
    out = tmp_path / "pick.csv"
    cmd = [pkg.CLI_PATH, "--program", "beta", "-t", "3", "--rng", "philox", "--logs", "0", "--sweep", "1000:3000:1000", "--out", str(tmp_path), "--pick", str(out)]
    spec = CLI_SPEC
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers)] + CLI_ARGS
    else:  # the defaults: the first 16 UEs by index, everybody
        spec = ((), "index", None, 16, ALL)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    assert out.read_bytes() == expected_csv(pkg, eng, spec)
    if workers == 1:
        bad = subprocess.run(cmd + ["--xtab", str(out)], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--pick cannot be combined" in bad.stdout
        bad = subprocess.run(cmd + ["--pick-where", "state:3:2"], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--pick-where FIELD:LO:HI" in bad.stdout


def test_sweep_driver_pick_two_ranks(pkg, eng, tmp_path):
    """sweep.py --pick with 2 ranks rehearsed on one GPU (gloo): the trials are gathered to rank 0, which writes them in trial order."""
    out = tmp_path / "pick.csv"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29547",
           os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--times", "3", "--sweep", "1000:3000:1000", "--out", str(tmp_path), "--backend", "gloo",
           "--same-device", "--pick", str(out)] + CLI_ARGS
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_bytes() == expected_csv(pkg, eng)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--pick", str(out), "--ci", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--pick cannot be combined" in bad.stderr
