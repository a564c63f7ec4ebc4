"""prach_run_trials_sojourn on the GPU: the sojourn histograms by arrival row prach::sojourn_kernel reduces on the device equal, integer for integer,
prach_sojourn_accumulate_logs of the per-UE logs the same call returns (`sojourn_from_logs`), a numpy restatement over those logs and — where an oracle run
is cheap — the same restatement over the oracle's UEs: behind every Beta.c / RandomAccessWithNOMA kernel, at the tile and window edges of the reduction
under both binning schemes, under every rerun the engine knows (a trial counts once), through groups, next to plain prach_run_trials and the other two
reductions, and through prach_sim --sojourn."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sojourn_ref as S  # noqa: E402
import timeline_ref as T  # noqa: E402
from kernel_matrix import ROWS  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0, sojourn_scheme=1)
ROW_NAMES = ("batch_w8_philox", "batch_w16_philox", "batch_glibc", "lcluster4_philox", "lcluster4_glibc", "cluster_wide_glibc", "legacy_philox")
SWEEP = (20, 500, 2002, 5)  # the CLI's default over Beta traffic: 500 ms rows over maxTime, 5 ms delay bins over maxTime + 6 ms


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def from_arrays(pkg, cfgs, arrays, spec, grp, ngroups):
    return S.numpy_sojourn(pkg, arrays, [pkg.arrival_schedule(c)[0] for c in cfgs], [c.accessTime for c in cfgs], spec, grp, ngroups)


def run_checked(pkg, eng, cfgs, spec, groups=None, ngroups=None):
    """One call with logs: the device's histograms equal sojourn_from_logs and numpy on the logs of the same call, and the sum identities hold."""
    res, logs, j = eng.run_trials_sojourn(cfgs, *spec, groups=groups, want_logs=True, ngroups=ngroups)
    assert all(r.status == 0 for r in res)
    grp = list(range(len(cfgs))) if groups is None else list(groups)
    host = pkg.sojourn_from_logs(cfgs, logs, *spec, groups=grp, ngroups=j.ngroups)
    assert j.same_as(host), (S.describe(j), S.describe(host))
    assert j.same_as(from_arrays(pkg, cfgs, [T.as_array(l) for l in logs], spec, grp, j.ngroups))
    sc = j.scalars
    assert int(sc["success"].sum()) == sum(r.nSuccessUE for r in res) and int(sc["arrived"].sum()) == sum(r.activeCheck for r in res)
    assert int(sc["trials"].sum()) == len(cfgs) and int(sc["ues"].sum()) == sum(c.nUE for c in cfgs)
    assert int(j.row_arrived.sum()) + int(sc["arrival_overflow"].sum()) == int(sc["arrived"].sum())
    tl = pkg.timeline_from_logs(cfgs, logs, spec[0], spec[1], groups=grp, ngroups=j.ngroups)  # the same arrival bins
    assert np.array_equal(j.hist.sum(axis=2) + j.row_delay_overflow, tl.series["success"]) and np.array_equal(j.row_arrived, tl.series["arrivals"])
    assert sc["sojourn_sum"].tolist() == tl.scalars["sojourn_sum"].tolist() and sc["restarted"].tolist() == tl.scalars["restarted"].tolist()
    return res, logs, j


def both_schemes(pkg, eng, cfgs, spec, groups=None, ngroups=None):
    """run_checked under sojourn_scheme 0 (global atomics only) and 1 (rows privatised in LDS): identical results."""
    eng.set("sojourn_scheme", 0)
    _, _, j0 = run_checked(pkg, eng, cfgs, spec, groups, ngroups)
    eng.set("sojourn_scheme", 1)
    res, logs, j1 = run_checked(pkg, eng, cfgs, spec, groups, ngroups)
    assert j1.same_as(j0)
    return res, logs, j1


_oracle = {}


def oracle_array(ob, c):
    key = bytes(c)
    if key not in _oracle:
        res, ues = ob.run_trial(T.oracle_cfg(ob, c), ob.Rng(c.rng_mode, c.seed))
        _oracle[key] = (res, T.as_array(ues).copy())
    return _oracle[key]


def equals_oracle(pkg, ob, cfgs, j, spec):
    exp = [oracle_array(ob, c) for c in cfgs]
    assert j.same_as(from_arrays(pkg, cfgs, [a for _, a in exp], spec, list(range(len(cfgs))), len(cfgs)))
    return [r for r, _ in exp]


@pytest.mark.parametrize("row", [r for r in ROWS if r["name"] in ROW_NAMES], ids=lambda r: r["name"])
def test_every_kernel_that_writes_the_log(pkg, ob, eng, row):
    """Each row's kernel, pinned by the row's options and prach_timing pins; nUE = 4097 and 5000, 12 grants.  A call counts only without a fallback trial."""
    assert len([r for r in ROWS if r["name"] in ROW_NAMES]) == len(ROW_NAMES)
    for k, v in dict(DEFAULTS, **row["opts"]).items():
        eng.set(k, v)
    cases = [(0, 4097, 11), (1, 5000, 12)]
    calls = [cases] if row["calls"] == "one_call" else [[c] for c in cases]
    counted = 0
    for call in calls:
        cfgs = [pkg.make_cfg(n, variant=v, rng_mode=row["rng"], seed=s, nGrantUL=12) for v, n, s in call]
        res, logs, j = both_schemes(pkg, eng, cfgs, SWEEP)
        tm = eng.timing()
        assert tm.sojourn_ms > 0 and tm.dist_ms == 0 and tm.timeline_ms == 0
        ores = equals_oracle(pkg, ob, cfgs, j, SWEEP)
        assert j.scalars["success"].tolist() == [r.nSuccessUE for r in ores] and j.scalars["arrived"].tolist() == [r.activeCheck for r in ores]
        if tm.fallback_trials == 0:
            assert {k: getattr(tm, k) for k in row["pin"]} == row["pin"] and tm.trial_kernel_reruns == 0
            counted += len(call)
    assert counted >= 1, "no call of this row stayed on its kernel"


def test_tile_edges_and_mixed_sizes_in_one_call(pkg, eng):
    tile = pkg.sojourn_tile_ues()
    sizes = [1, 37, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 4099]  # (trials of different nUE side by side: every job boundary is a workgroup's)
    cfgs = [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate(sizes)]
    both_schemes(pkg, eng, cfgs, SWEEP)
    both_schemes(pkg, eng, cfgs, (1, 10006, 10006, 1))
    eng.set("cluster", 4)  # the cluster kernels' log, one call per trial
    for k, n in enumerate(sizes):
        both_schemes(pkg, eng, [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=40 + k)], SWEEP)
        tm = eng.timing()
        assert tm.cluster_size == 4 or tm.fallback_trials > 0


def test_windows(pkg, ob, eng):
    words = pkg.sojourn_window_words()
    wide = pkg.make_cfg(8000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=9)
    spec = (4096, 2, 64, 200)  # 2 ms rows: far more rows than the window holds
    _, logs, j = both_schemes(pkg, eng, [wide], spec)
    at, _, ok, soj = S.sojourns(T.as_array(logs[0]), pkg.arrival_schedule(wide)[0], 5)
    assert int(at[-1] - at[0]) == 6650 and 6650 // 2 > words // 64  # one tile whose arrival rows alone leave the LDS window: the rest goes to the global cells
    equals_oracle(pkg, ob, [wide], j, spec)
    _, _, j = both_schemes(pkg, eng, [wide], (4096, 1, 64, 200))  # 1 ms rows: arrivals behind 4096 ms are in no row
    assert int(j.scalars["arrival_overflow"][0]) > 0
    equals_oracle(pkg, ob, [wide], j, (4096, 1, 64, 200))
    fit = words // 64  # exactly as many rows as the window holds, over the whole horizon; then a row more
    for rows in (fit, fit + 1):
        spec = (rows, -(-10006 // rows), 64, 200)
        _, _, j = both_schemes(pkg, eng, [wide], spec)
        assert int(j.scalars["arrival_overflow"][0]) == 0
        equals_oracle(pkg, ob, [wide], j, spec)
    for rows, rw in ((1, 10006), (21, 500)):  # 16384 bins of 1 ms: the window holds one row at most
        assert words // 16384 <= 1
        _, _, j = both_schemes(pkg, eng, [wide], (rows, rw, 16384, 1))
        assert int(j.scalars["delay_overflow"][0]) == 0
    _, _, j = both_schemes(pkg, eng, [wide], (4096, 2, 7, 2000))  # every row privatised next to a full window: the kernel's largest LDS layout
    assert 4096 * 7 == words and int(j.scalars["arrival_overflow"][0]) == 0 and int(j.scalars["delay_overflow"][0]) == 0
    _, _, j = both_schemes(pkg, eng, [wide], (1, 1, 1, 1))  # one cell: who arrives in the first millisecond and completes within it
    assert int(j.scalars["arrival_overflow"][0]) > 7000 and int(j.scalars["delay_overflow"][0]) == int(j.scalars["success"][0])
    spec = (21, 500, 40, 5)  # a delay range below the largest sojourn: overflow per row
    _, _, j = both_schemes(pkg, eng, [wide], spec)
    assert int(soj[ok].max()) >= 200 and int(j.row_delay_overflow.sum()) == int(j.scalars["delay_overflow"][0]) > 0 and (j.row_delay_overflow[0] > 0).sum() > 3
    equals_oracle(pkg, ob, [wide], j, spec)
    top = int(soj[ok].max())  # the delay range ends exactly at the largest sojourn: that UE is in the FIRST bin of the overflow, and the only one there
    for w in (1, 5):
        spec = (21, 500, top // w, w)
        _, _, j = both_schemes(pkg, eng, [wide], spec)
        assert int(j.scalars["delay_overflow"][0]) == int((soj[ok] // w >= top // w).sum()) >= 1 and int(j.scalars["sojourn_max"][0]) == top
        equals_oracle(pkg, ob, [wide], j, spec)
    uni = pkg.make_cfg(1000, variant=0, uniform=1, rng_mode=pkg.RNG_PHILOX, seed=1)  # Uniform traffic over 60 000 ms
    spec = (4096, 15, 256, 4)
    _, _, j = both_schemes(pkg, eng, [uni], spec)
    assert int(j.scalars["arrival_overflow"][0]) == 0 and np.flatnonzero(j.row_arrived[0])[-1] > 2 * (words // 256)
    equals_oracle(pkg, ob, [uni], j, spec)
    for access_time, rw in ((1, 3), (7, 3), (7, 5)):  # a row width that does not divide the access slot
        c = pkg.make_cfg(3000, variant=access_time % 2, rng_mode=pkg.RNG_PHILOX, seed=access_time, accessTime=access_time)
        spec = (-(-10006 // rw), rw, 300, 7)
        _, _, j = both_schemes(pkg, eng, [c], spec)
        equals_oracle(pkg, ob, [c], j, spec)


def test_overloaded_trial(pkg, ob, eng):
    """Most successful UEs started over: the time since arrival is tens of times the reference's `timer` (842 947 ms in all)."""
    c = pkg.make_cfg(20000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=7, maxMsg2TxCount=3)
    res, _, j = both_schemes(pkg, eng, [c], SWEEP)
    sc = {f: int(v[0]) for f, v in j.scalars.items()}
    equals_oracle(pkg, ob, [c], j, SWEEP)
    assert (sc["success"], sc["sojourn_sum"], sc["restarted"]) == (17782, 30210018, 15381) and res[0].sumTimer == 842947
    assert j.quantile(0, -1, 0.5) * 10 > sc["sojourn_sum"] // sc["success"] > 10 * (842947 // 17782)


def test_truncated_trial_counts_arrived_ues_only(pkg, ob, eng):
    for rng in (pkg.RNG_GLIBC, pkg.RNG_PHILOX):
        c = pkg.make_cfg(8000, variant=1, rng_mode=rng, seed=9, max_steps=2500)
        res, logs, j = both_schemes(pkg, eng, [c], SWEEP)
        (ores,) = equals_oracle(pkg, ob, [c], j, SWEEP)
        assert int(j.scalars["arrived"][0]) == res[0].activeCheck == ores.activeCheck < 8000 and int(j.scalars["success"][0]) == ores.nSuccessUE
        assert (T.as_array(logs[0])[:, T.ACTIVE] == -1).sum() == 8000 - ores.activeCheck
    assert ores.activeCheck == 1646


def undisturbed_then(pkg, cfgs, disturb):
    """The histograms of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, j = run_checked(pkg, e, cfgs, SWEEP, groups=[k % 2 for k in range(len(cfgs))] if len(cfgs) > 1 else None)
            out.append((j, e.timing()))
        finally:
            e.close()
    (a, t0), (b, t1) = out
    assert b.same_as(a) and int(b.scalars["trials"].sum()) == len(cfgs)
    return t0, t1


def test_counted_once_calendar_rerun(pkg):
    cases = [(3000, {}), (8000, dict(nGrantUL=3)), (12000, dict(nGrantUL=2))]  # the shapes of test_calendar_cap_rerun_is_exact
    cfgs = [pkg.make_cfg(n, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s, **kw) for s in (0, 1) for n, kw in cases]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("calendar_cap", 64))
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1.launches > t0.launches


def test_counted_once_mem_budget_split(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(8) for v in (0, 1) for n in (3000, 6000)]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("mem_budget_mb", 64))
    assert t1.launches >= 2 and t1.launches > t0.launches  # (the device logs of every trial count against the budget like the rest of the arena)


def test_counted_once_stream_retry(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_GLIBC, seed=s) for n, v, s in ((5000, 0, 1), (5000, 1, 2), (20000, 1, 3))]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("stream_factor", 1))
    assert t1.launches > t0.launches  # (a window of one draw per UE runs out: the trials are run again with a larger one)


def test_counted_once_resident_hook(pkg):
    cfgs = [pkg.make_cfg(20000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3)]  # the shapes of test_cluster_residency_is_explicit

    def narrow(e):
        e.set("cluster", 16)
        e.set("resident", 30)
    t0, t1 = undisturbed_then(pkg, cfgs, narrow)
    assert t1.resident_limit == 30 and t1.cluster_size == 8


def test_groups(pkg, eng):
    rng = np.random.default_rng(3)
    cfgs = [pkg.make_cfg(int(n), variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate(rng.integers(500, 3000, 40))]  # unequal nUE in every group
    groups = rng.permutation(np.arange(40) % 3).tolist()
    _, _, j3 = both_schemes(pkg, eng, cfgs, SWEEP, groups=groups)
    _, _, j5 = run_checked(pkg, eng, cfgs, SWEEP, groups=[g if g < 2 else 4 for g in groups], ngroups=6)  # groups 2, 3 and 5 have no trial
    for g in (2, 3, 5):
        assert int(j5.scalars["sojourn_max"][g]) == -1 and not any(a[g].any() for a in j5._arrays())
        assert [int(j5.scalars[f][g]) for f in pkg.SOJOURN_FIELDS[:-1]] == [0] * 8
    _, _, per_trial = run_checked(pkg, eng, cfgs, SWEEP)  # identity grouping, a second call
    merged = pkg.Sojourn(3, *SWEEP)
    for k, g in enumerate(groups):
        merged.merge_group(g, per_trial, k)
    assert merged.same_as(j3)  # merged on the device == prach_sojourn_merge of the per-trial results
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_sojourn(cfgs, *SWEEP, groups=[0] * 39 + [3], ngroups=3)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_sojourn(cfgs, *SWEEP, ngroups=39)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c: refused before anything is launched
        eng.run_trials_sojourn(cfgs[:2] + [pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1)], *SWEEP)
    assert ei.value.status == -2


def test_isolation_from_plain_run_trials(pkg, eng):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s) for n, v, r, s in ((3000, 0, 1, 1), (5000, 1, 1, 2), (4000, 1, 0, 3))]
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().sojourn_ms == 0
    res1, logs1, _ = eng.run_trials_sojourn(cfgs, *SWEEP, want_logs=True)
    assert eng.timing().sojourn_ms > 0
    res2, logs2 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().sojourn_ms == 0
    for res, logs in ((res1, logs1), (res2, logs2)):
        assert [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert all(bytes(a) == bytes(b) for a, b in zip(logs, logs0))
    exp = pkg.sojourn_from_logs(cfgs, logs0, *SWEEP)
    _, nologs, j = eng.run_trials_sojourn(cfgs, *SWEEP)  # without host logs: the same histograms
    assert nologs == [None] * 3 and j.same_as(exp)
    _, some, j = eng.run_trials_sojourn(cfgs, *SWEEP, want_logs=[1])  # ... and with the log of one trial only
    assert some[0] is None and some[2] is None and bytes(some[1]) == bytes(logs0[1]) and j.same_as(exp)


def test_three_reductions_alternate_on_one_engine(pkg, eng):
    """The three reductions share one device buffer, one job table and one pair of events: they alternate on one engine — a small buffer after a large one
    (anything stale or unzeroed would show), then growing ones.  Each equals the host-side definition over the logs of its own call, leaves the other two
    *_ms at 0, and the results of all calls are the same."""
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate((300, 8192, 8193))]  # the edges of the kernels' tile
    cfgs.append(pkg.make_cfg(2000, variant=pkg.VARIANT_WITHNOMA_C, rng_mode=pkg.RNG_PHILOX, seed=3, maxMsg2TxCount=3))  # some UEs start over
    steps = [("sojourn", (21, 500, 2002, 5), [0, 1, 2, 0]), ("dist", (16, 1), [0, 0, 0, 0]), ("sojourn", (2, 5003, 8, 100), None), ("timeline", (10006, 1), None),
             ("sojourn", (100, 101, 10006, 1), [1, 1, 0, 0]), ("dist", (16384, 1), None), ("timeline", (2002, 5), [0, 1, 2, 0]), ("sojourn", (1, 1, 1, 1), None)]
    all_res = []
    for kind, params, groups in steps:
        res, logs, red = getattr(eng, "run_trials_" + kind)(cfgs, *params, groups=groups, want_logs=True)
        tm = eng.timing()
        assert all(r.status == 0 for r in res)
        ms = dict(sojourn=tm.sojourn_ms, dist=tm.dist_ms, timeline=tm.timeline_ms)
        assert ms.pop(kind) > 0 and list(ms.values()) == [0, 0]
        if kind == "dist":
            host = pkg.dist_from_logs(logs, *params, groups=groups)
        else:
            host = getattr(pkg, kind + "_from_logs")(cfgs, logs, *params, groups=groups)
            assert int(red.scalars["restarted"].sum()) > 0
        assert red.ngroups == host.ngroups == (4 if groups is None else max(groups) + 1) and red.same_as(host)
        all_res.append(res)
    res, _ = eng.run_trials(cfgs)
    tm = eng.timing()
    assert tm.dist_ms == 0 and tm.timeline_ms == 0 and tm.sojourn_ms == 0
    all_res.append(res)
    for res in all_res[1:]:
        assert [r.as_dict() for r in res] == [r.as_dict() for r in all_res[0]]


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_sojourn_equals_the_logs(pkg, eng, tmp_path, workers):
    """prach_sim --sojourn with --logs 0 on a shortened sweep, three seeds per point merged — and the same from two forked workers on one device."""
    out = tmp_path / "sojourn.csv"
    cmd = [pkg.CLI_PATH, "--program", "beta", "-t", "3", "--rng", "philox", "--logs", "0", "--sweep", "2000:6000:2000", "--out", str(tmp_path), "--sojourn", str(out)]
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [2000, 4000, 6000]
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in points]
    _, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.sojourn_from_logs(cfgs, logs, *SWEEP, groups=[k % 3 for k in range(9)], ngroups=3)  # the CLI's default: 500 ms rows, 5 ms bins over maxTime + 6 ms
    assert out.read_bytes() == pkg.sojourn_csv(exp, labels=points) and len(out.read_bytes()) > 1000


def test_sweep_driver_sojourn_two_ranks(pkg, eng, tmp_path):
    """sweep.py --sojourn with 2 ranks rehearsed on one GPU (gloo): every rank's groups merged by allreduce_sojourn, rank 0 writes the CSV of the logs."""
    out = tmp_path / "sojourn.csv"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29541",
           os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--times", "3", "--sweep", "2000:6000:2000", "--out", str(tmp_path), "--backend", "gloo",
           "--same-device", "--sojourn", str(out), "--sojourn-arrival-ms", "1000", "--sojourn-bin", "10"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    points = [2000, 4000, 6000]
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in points]
    _, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.sojourn_from_logs(cfgs, logs, 10, 1000, 1001, 10, groups=[k % 3 for k in range(9)], ngroups=3)
    assert out.read_bytes() == pkg.sojourn_csv(exp, labels=points) and len(out.read_bytes()) > 1000
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--sojourn", str(out), "--timeline", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--sojourn cannot be combined" in bad.stderr
