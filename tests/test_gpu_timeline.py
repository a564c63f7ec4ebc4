"""prach_run_trials_timeline on the GPU: the timelines prach::timeline_kernel reduces on the device equal, integer for integer, prach_timeline_accumulate_logs
of the per-UE logs the same call returns (`timeline_from_logs`), a numpy restatement over those logs and — where an oracle run is cheap — the same
restatement over the oracle's UEs: behind every Beta.c / RandomAccessWithNOMA kernel, at the tile and window edges of the reduction under both binning
schemes, under every rerun the engine knows (a trial counts once), through groups, next to plain prach_run_trials, and through prach_sim --timeline."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import timeline_ref as T  # noqa: E402
from kernel_matrix import ROWS  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0, timeline_scheme=1)
ROW_NAMES = ("batch_w8_philox", "batch_w16_philox", "batch_glibc", "lcluster4_philox", "lcluster4_glibc", "cluster_wide_glibc", "legacy_philox")


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def horizon(c, width):
    return -(-((60000 if c.uniform else 10000) + 6) // width)


def from_arrays(pkg, cfgs, arrays, bins, width, grp, ngroups):
    return T.numpy_timeline(pkg, arrays, [pkg.arrival_schedule(c)[0] for c in cfgs], [c.accessTime for c in cfgs], bins, width, grp, ngroups)


def run_checked(pkg, eng, cfgs, bins, width=1, groups=None, ngroups=None):
    """One call with logs: the device's timelines equal timeline_from_logs and numpy on the logs of the same call, and the results' own sums."""
    res, logs, t = eng.run_trials_timeline(cfgs, bins, width, groups=groups, want_logs=True, ngroups=ngroups)
    assert all(r.status == 0 for r in res)
    grp = list(range(len(cfgs))) if groups is None else list(groups)
    host = pkg.timeline_from_logs(cfgs, logs, bins, width, groups=grp, ngroups=t.ngroups)
    assert t.same_as(host), (T.describe(t), T.describe(host))
    assert t.same_as(from_arrays(pkg, cfgs, [T.as_array(l) for l in logs], bins, width, grp, t.ngroups))
    sc = t.scalars
    assert int(sc["timer_sum"].sum()) == sum(r.sumTimer for r in res) and int(sc["success"].sum()) == sum(r.nSuccessUE for r in res)
    assert int(sc["arrived"].sum()) == sum(r.activeCheck for r in res) and int(sc["trials"].sum()) == len(cfgs) and int(sc["ues"].sum()) == sum(c.nUE for c in cfgs)
    assert int(t.series["arrivals"].sum()) + int(sc["arrival_overflow"].sum()) == int(sc["arrived"].sum())
    assert int(t.series["done"].sum()) + int(sc["done_overflow"].sum()) == int(sc["success"].sum())
    return res, logs, t


def both_schemes(pkg, eng, cfgs, bins, width=1, groups=None, ngroups=None):
    """run_checked under timeline_scheme 0 (global atomics only) and 1 (LDS windows): identical results."""
    eng.set("timeline_scheme", 0)
    _, _, t0 = run_checked(pkg, eng, cfgs, bins, width, groups, ngroups)
    eng.set("timeline_scheme", 1)
    res, logs, t1 = run_checked(pkg, eng, cfgs, bins, width, groups, ngroups)
    assert t1.same_as(t0)
    return res, logs, t1


_oracle = {}


def oracle_array(ob, c):
    key = bytes(c)
    if key not in _oracle:
        res, ues = ob.run_trial(T.oracle_cfg(ob, c), ob.Rng(c.rng_mode, c.seed))
        _oracle[key] = (res, T.as_array(ues).copy())
    return _oracle[key]


def equals_oracle(pkg, ob, cfgs, t, bins, width):
    exp = [oracle_array(ob, c) for c in cfgs]
    assert t.same_as(from_arrays(pkg, cfgs, [a for _, a in exp], bins, width, list(range(len(cfgs))), len(cfgs)))
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
        res, logs, t = both_schemes(pkg, eng, cfgs, 2048, 5)
        tm = eng.timing()
        assert tm.timeline_ms > 0 and tm.dist_ms == 0
        ores = equals_oracle(pkg, ob, cfgs, t, 2048, 5)
        assert t.scalars["timer_sum"].tolist() == [r.sumTimer for r in ores] and t.scalars["arrived"].tolist() == [r.activeCheck for r in ores]
        if tm.fallback_trials == 0:
            assert {k: getattr(tm, k) for k in row["pin"]} == row["pin"] and tm.trial_kernel_reruns == 0
            counted += len(call)
    assert counted >= 1, "no call of this row stayed on its kernel"


def test_tile_edges_and_mixed_sizes_in_one_call(pkg, eng):
    tile = pkg.timeline_tile_ues()
    sizes = [1, 37, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 4099]  # (trials of different nUE side by side: every job boundary is a workgroup's)
    cfgs = [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate(sizes)]
    both_schemes(pkg, eng, cfgs, 2002, 5)
    both_schemes(pkg, eng, cfgs, 10006, 1)
    eng.set("cluster", 4)  # the cluster kernels' log, one call per trial
    for k, n in enumerate(sizes):
        both_schemes(pkg, eng, [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=40 + k)], 2002, 5)
        tm = eng.timing()
        assert tm.cluster_size == 4 or tm.fallback_trials > 0


def test_windows(pkg, ob, eng):
    window = pkg.timeline_window_bins()
    wide = pkg.make_cfg(8000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=9)
    _, logs, t = both_schemes(pkg, eng, [wide], 10006, 1)
    at, _, _, _ = T.per_ue(T.as_array(logs[0]), pkg.arrival_schedule(wide)[0], 5)
    assert int(at[-1] - at[0]) == 6650 > window  # one tile whose arrivals alone leave the LDS window: the rest goes to the global bins directly
    equals_oracle(pkg, ob, [wide], t, 10006, 1)
    _, _, t = both_schemes(pkg, eng, [wide], 202, 50)  # the same trial inside the window
    assert int((at[-1] - at[0]) // 50) < window and int(t.scalars["arrival_overflow"][0]) == 0 and int(t.scalars["done_overflow"][0]) == 0
    equals_oracle(pkg, ob, [wide], t, 202, 50)
    _, _, t = both_schemes(pkg, eng, [wide], 1, 1)  # one bin: only what arrives and completes in the first millisecond
    assert int(t.scalars["arrival_overflow"][0]) > 7000
    _, _, t = both_schemes(pkg, eng, [wide], 300, 10)  # bins x width below the horizon: both axes overflow
    assert int(t.scalars["arrival_overflow"][0]) > 0 and int(t.scalars["done_overflow"][0]) > 0
    equals_oracle(pkg, ob, [wide], t, 300, 10)
    uni = pkg.make_cfg(1000, variant=0, uniform=1, rng_mode=pkg.RNG_PHILOX, seed=1)  # Uniform traffic over 60 000 ms at 1 ms
    _, _, t = both_schemes(pkg, eng, [uni], 60006, 1)
    assert int(t.scalars["arrival_overflow"][0]) == 0 and int(t.scalars["done_overflow"][0]) == 0 and np.flatnonzero(t.series["arrivals"][0])[-1] > 2 * window
    equals_oracle(pkg, ob, [uni], t, 60006, 1)
    for access_time, width in ((1, 3), (7, 3), (7, 5)):  # a width that does not divide the access slot
        c = pkg.make_cfg(3000, variant=access_time % 2, rng_mode=pkg.RNG_PHILOX, seed=access_time, accessTime=access_time)
        _, _, t = both_schemes(pkg, eng, [c], horizon(c, width), width)
        equals_oracle(pkg, ob, [c], t, horizon(c, width), width)


def test_overloaded_trial_restarts(pkg, ob, eng):
    """The reference's access delay is the length of the LAST attempt cycle: here most successful UEs started over, and the time since arrival is tens of
    times the timer (the oracle: 15 381 of 17 782 UEs, 30 210 018 ms against 842 947 ms)."""
    c = pkg.make_cfg(20000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=7, maxMsg2TxCount=3)
    _, _, t = both_schemes(pkg, eng, [c], 2002, 5)
    sc = {f: int(v[0]) for f, v in t.scalars.items()}
    assert sc["restarted"] > sc["success"] // 2 and sc["sojourn_sum"] > 10 * sc["timer_sum"]
    equals_oracle(pkg, ob, [c], t, 2002, 5)
    assert (sc["success"], sc["restarted"], sc["timer_sum"], sc["sojourn_sum"], sc["done_max"]) == (17782, 15381, 842947, 30210018, 10003)


def test_truncated_trial_counts_arrived_ues_only(pkg, ob, eng):
    for rng in (pkg.RNG_GLIBC, pkg.RNG_PHILOX):
        c = pkg.make_cfg(8000, variant=1, rng_mode=rng, seed=9, max_steps=2500)
        res, logs, t = both_schemes(pkg, eng, [c], 2002, 5)
        (ores,) = equals_oracle(pkg, ob, [c], t, 2002, 5)
        assert int(t.scalars["arrived"][0]) == res[0].activeCheck == ores.activeCheck < 8000 and int(t.scalars["success"][0]) == ores.nSuccessUE
        assert (T.as_array(logs[0])[:, T.ACTIVE] == -1).sum() == 8000 - ores.activeCheck
    assert ores.activeCheck == 1646


def undisturbed_then(pkg, cfgs, disturb):
    """The timelines of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, t = run_checked(pkg, e, cfgs, 2002, 5, groups=[k % 2 for k in range(len(cfgs))] if len(cfgs) > 1 else None)
            out.append((t, e.timing()))
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
    cfgs = [pkg.make_cfg(int(n), variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate(rng.integers(500, 3000, 40))]
    groups = rng.permutation(np.arange(40) % 3).tolist()
    _, _, t3 = both_schemes(pkg, eng, cfgs, 2002, 5, groups=groups)
    _, _, t5 = run_checked(pkg, eng, cfgs, 2002, 5, groups=[g if g < 2 else 4 for g in groups], ngroups=6)  # groups 2, 3 and 5 have no trial
    for g in (2, 3, 5):
        assert int(t5.scalars["done_max"][g]) == -1 and not any(t5.series[n][g].any() for n in pkg.TIMELINE_SERIES)
        assert [int(t5.scalars[f][g]) for f in pkg.TIMELINE_FIELDS[:-1]] == [0] * 9
    _, _, per_trial = run_checked(pkg, eng, cfgs, 2002, 5)  # identity grouping, a second call
    merged = pkg.Timeline(3, 2002, 5)
    for k, g in enumerate(groups):
        merged.merge_group(g, per_trial, k)
    assert merged.same_as(t3)  # merged on the device == prach_timeline_merge of the per-trial results
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_timeline(cfgs, 2002, 5, groups=[0] * 39 + [3], ngroups=3)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_timeline(cfgs, 2002, 5, ngroups=39)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c: refused before anything is launched
        eng.run_trials_timeline(cfgs[:2] + [pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1)], 2002, 5)
    assert ei.value.status == -2


def test_isolation_from_plain_run_trials(pkg, eng):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s) for n, v, r, s in ((3000, 0, 1, 1), (5000, 1, 1, 2), (4000, 1, 0, 3))]
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().timeline_ms == 0
    res1, logs1, _ = eng.run_trials_timeline(cfgs, 2002, 5, want_logs=True)
    assert eng.timing().timeline_ms > 0
    res2, logs2 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().timeline_ms == 0
    for res, logs in ((res1, logs1), (res2, logs2)):
        assert [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert all(bytes(a) == bytes(b) for a, b in zip(logs, logs0))
    exp = pkg.timeline_from_logs(cfgs, logs0, 2002, 5)
    _, nologs, t = eng.run_trials_timeline(cfgs, 2002, 5)  # without host logs: the same timelines
    assert nologs == [None] * 3 and t.same_as(exp)
    _, some, t = eng.run_trials_timeline(cfgs, 2002, 5, want_logs=[1])  # ... and with the log of one trial only
    assert some[0] is None and some[2] is None and bytes(some[1]) == bytes(logs0[1]) and t.same_as(exp)


@pytest.mark.parametrize("workers", [1, 4])
def test_cli_timeline_equals_the_logs(pkg, eng, tmp_path, workers):
    """prach_sim --timeline with --logs 0 on a shortened sweep, three seeds per point merged — and the same from four forked workers on one device."""
    out = tmp_path / "timeline.csv"
    cmd = [pkg.CLI_PATH, "--program", "beta", "-t", "3", "--rng", "philox", "--logs", "0", "--sweep", "2000:6000:2000", "--out", str(tmp_path), "--timeline", str(out)]
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [2000, 4000, 6000]
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in points]
    _, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.timeline_from_logs(cfgs, logs, 2002, 5, groups=[k % 3 for k in range(9)], ngroups=3)  # the CLI's default: 5 ms bins over maxTime + 6 ms
    assert out.read_bytes() == pkg.timeline_csv(exp, labels=points) and len(out.read_bytes()) > 1000


def test_alternating_reductions_share_one_engine(pkg, eng):
    """The two reductions of an engine share one device buffer, one job table and one pair of events: timeline and dist calls alternate on one engine —
    a small buffer after a large one (anything stale or unzeroed would show), then growing ones — and a plain call ends the row.  Every reduction equals
    the host-side definition over the logs of its own call and the same call on an engine that has made no other; the results of all calls are the same."""
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate((300, 8192, 8193))]  # the edges of both kernels' tile
    cfgs.append(pkg.make_cfg(2000, variant=pkg.VARIANT_WITHNOMA_C, rng_mode=pkg.RNG_PHILOX, seed=3, maxMsg2TxCount=3))  # some UEs start over
    assert pkg.timeline_tile_ues() == pkg.dist_tile_ues() == 8192
    steps = [("timeline", (horizon(cfgs[0], 5), 5), [0, 1, 2, 0]), ("dist", (16, 1), [0, 0, 0, 0]), ("timeline", (horizon(cfgs[0], 1), 1), None),
             ("dist", (16384, 1), None)]
    all_res = []
    for kind, params, groups in steps:
        def call(e):
            return (e.run_trials_timeline if kind == "timeline" else e.run_trials_dist)(cfgs, *params, groups=groups, want_logs=True)
        res, logs, red = call(eng)
        tm = eng.timing()
        assert all(r.status == 0 for r in res)
        if kind == "timeline":
            assert tm.timeline_ms > 0 and tm.dist_ms == 0
            host = pkg.timeline_from_logs(cfgs, logs, *params, groups=groups)
            assert int(red.scalars["restarted"].sum()) > 0
        else:
            assert tm.dist_ms > 0 and tm.timeline_ms == 0
            host = pkg.dist_from_logs(logs, *params, groups=groups)
        assert red.ngroups == host.ngroups == (4 if groups is None else max(groups) + 1) and red.same_as(host)
        fresh = pkg.Engine(0)
        try:
            assert red.same_as(call(fresh)[2])
        finally:
            fresh.close()
        all_res.append(res)
    res, _ = eng.run_trials(cfgs)
    tm = eng.timing()
    assert tm.dist_ms == 0 and tm.timeline_ms == 0
    all_res.append(res)
    assert len(all_res) == 5
    for res in all_res[1:]:
        assert [r.as_dict() for r in res] == [r.as_dict() for r in all_res[0]]
