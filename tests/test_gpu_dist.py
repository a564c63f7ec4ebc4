"""prach_run_trials_dist on the GPU: the distributions prach::dist_kernel reduces on the device equal, integer for integer, prach_dist_accumulate_logs of
the per-UE logs the same call returns (`dist_from_logs`) and np.bincount of the oracle's UEs — behind every kernel that leaves final state, at the
shape edges of the reduction, under every rerun the engine knows (a trial counts once), through groups, and through prach_sim --cdf."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from kernel_matrix import ROWS  # noqa: E402
from reduce_cases import bincount_dist  # noqa: E402  (np.bincount form of the distributions over int32 [nUE, 16] per-UE arrays)

pytestmark = pytest.mark.gpu

TIMER, PTC, FLAG = 1, 11, 14
NOMA_UE = np.dtype([("i", np.int32, 16), ("g", np.float64)])
DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0, dist_scheme=1)
ROW_NAMES = ("batch_w8_philox", "batch_w16_philox", "batch_glibc", "lcluster4_philox", "lcluster4_glibc", "cluster_wide_glibc", "noma1_philox", "noma4_philox",
             "noma_glibc", "legacy_philox")


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def as_array(log):
    return np.frombuffer(log, dtype=np.int32).reshape(-1, 16)


def describe(d):
    return {f: getattr(d, f).tolist() for f in ("trials", "ues", "success", "delay_overflow", "delay_sum", "ptc_sum", "delay_max")}


def run_checked(pkg, eng, cfgs, bins, width=1, groups=None, ngroups=None):
    """One call with logs: the device's distributions equal dist_from_logs and np.bincount of the logs of the same call, and the results' own sums."""
    res, logs, d = eng.run_trials_dist(cfgs, bins, width, groups=groups, want_logs=True, ngroups=ngroups)
    assert all(r.status == 0 for r in res)
    grp = list(range(len(cfgs))) if groups is None else list(groups)
    host = pkg.dist_from_logs(logs, bins, width, groups=grp, ngroups=d.ngroups)
    assert d.same_as(host), (describe(d), describe(host))
    assert d.same_as(bincount_dist(pkg, [as_array(l) for l in logs], bins, width, grp, d.ngroups))
    assert int(d.delay_sum.sum()) == sum(r.sumTimer for r in res) and int(d.ptc_sum.sum()) == sum(r.preambleTxCount for r in res)
    assert int(d.success.sum()) == sum(r.nSuccessUE for r in res) and int(d.trials.sum()) == len(cfgs) and int(d.ues.sum()) == sum(c.nUE for c in cfgs)
    return res, logs, d


_oracle = {}


def oracle_ues(ob, program, variant, n, rng, seed):
    key = (program, variant, n, rng, seed)
    if key not in _oracle:
        if program == "noma":
            res, ues = ob.noma_run_trial(ob.make_noma_cfg(n, nGrantUL=12), ob.Rng(rng, seed))
            _oracle[key] = (np.frombuffer(ues, dtype=NOMA_UE)["i"].copy(), res.delay, res.nTxP)
        else:
            res, ues = ob.run_trial(ob.make_cfg(n, variant=variant, nGrantUL=12), ob.Rng(rng, seed))
            _oracle[key] = (as_array(ues).copy(), res.sumTimer, res.preambleTxCount)
    return _oracle[key]


@pytest.mark.parametrize("row", [r for r in ROWS if r["name"] in ROW_NAMES], ids=lambda r: r["name"])
def test_every_kernel_that_leaves_final_state(pkg, ob, eng, row):
    """Each row's kernel, pinned by the row's options and prach_timing pins; nUE = 4097 and 5000, 12 grants.  A call counts only without a fallback trial."""
    assert len([r for r in ROWS if r["name"] in ROW_NAMES]) == len(ROW_NAMES)
    for k, v in dict(DEFAULTS, **row["opts"]).items():
        eng.set(k, v)
    if row["program"] == "noma":
        cases = [("noma", 2, 4097, 5), ("noma", 2, 5000, 6)]
    else:
        cases = [("beta", 0, 4097, 11), ("beta", 1, 5000, 12)]
    calls = [cases] if row["calls"] == "one_call" else [[c] for c in cases]
    counted = 0
    for call in calls:
        cfgs = [pkg.make_cfg(n, variant=v, rng_mode=row["rng"], seed=s, nGrantUL=12) for _, v, n, s in call]
        res, logs, d = run_checked(pkg, eng, cfgs, 4096)
        tm = eng.timing()
        assert tm.dist_ms > 0
        exp = [oracle_ues(ob, prog, v, n, row["rng"], s) for prog, v, n, s in call]
        assert d.same_as(bincount_dist(pkg, [e[0] for e in exp], 4096, 1, range(len(call)), len(call)))
        assert d.delay_sum.tolist() == [e[1] for e in exp] and d.ptc_sum.tolist() == [e[2] for e in exp]
        if tm.fallback_trials == 0:
            assert {k: getattr(tm, k) for k in row["pin"]} == row["pin"] and tm.trial_kernel_reruns == 0
            counted += len(call)
    assert counted >= 1, "no call of this row stayed on its kernel"


def test_shape_edges_and_mixed_sizes_in_one_call(pkg, eng):
    tile = pkg.dist_tile_ues()
    sizes = [1, 37, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 63, 1000, 4099]  # (trials of different nUE side by side: every job boundary is a workgroup's)
    cfgs = [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate(sizes)]
    run_checked(pkg, eng, cfgs, 1024)
    eng.set("cluster", 4)  # the int32-array form of the preamble counts (the cluster kernels), one call per trial
    for k, n in enumerate((tile - 1, tile, tile + 1, 2 * tile + 1)):
        run_checked(pkg, eng, [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=40 + k)], 1024)
        assert eng.timing().rec_mode != 4


@pytest.fixture(scope="module")
def overloaded(pkg):
    """The overloaded 20 000-UE trial: 12 grants serve a fraction of the UEs, nearly every successful one after 1..4 preambles (maxMsg2TxCount = 3)."""
    return [pkg.make_cfg(20000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=7, maxMsg2TxCount=3)]


@pytest.mark.parametrize("bins,width", [(1, 1), (8, 5), (16384, 1), (700, 7)])
def test_bins(pkg, eng, overloaded, bins, width):
    _, logs, d = run_checked(pkg, eng, overloaded, bins, width)
    delays = as_array(logs[0])[as_array(logs[0])[:, FLAG] == 1, TIMER]
    assert delays.size > 1000
    if (bins, width) == (8, 5):
        assert int(d.delay_overflow[0]) > delays.size // 2  # most delays overflow 40 ms
    if bins == 16384:
        assert int(d.delay_overflow[0]) == 0 and int(d.delay_max[0]) == int(delays.max())
        assert pkg.dist_quantile(d, 0, 0.5) == int(np.sort(delays)[-(-delays.size // 2) - 1])
    if width == 7:
        assert (delays % 7 != 0).any()


@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_contention_every_binning_scheme(pkg, eng, overloaded, scheme):
    eng.set("dist_scheme", scheme)
    _, _, d = run_checked(pkg, eng, overloaded, 4096)
    top4 = np.sort(d.ptc_hist[0])[-4:].sum()
    assert int(top4) >= 0.9 * int(d.success[0]) > 900  # nearly every successful UE in four bins


def test_groups(pkg, eng):
    rng = np.random.default_rng(3)
    cfgs = [pkg.make_cfg(int(n), variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k) for k, n in enumerate(rng.integers(500, 3000, 40))]
    groups = rng.permutation(np.arange(40) % 3).tolist()
    _, _, d3 = run_checked(pkg, eng, cfgs, 2048, 1, groups=groups)
    _, _, d5 = run_checked(pkg, eng, cfgs, 2048, 1, groups=[g if g < 2 else 4 for g in groups], ngroups=6)  # groups 2, 3 and 5 have no trial
    for g in (2, 3, 5):
        assert int(d5.delay_max[g]) == -1 and not d5.delay_hist[g].any() and not d5.ptc_hist[g].any()
        assert [int(getattr(d5, f)[g]) for f in ("trials", "ues", "success", "delay_overflow", "delay_sum", "ptc_sum")] == [0] * 6
    _, _, per_trial = run_checked(pkg, eng, cfgs, 2048, 1)  # identity grouping, a second call
    merged = pkg.Dist(3, 2048, 1)
    for k, g in enumerate(groups):
        merged.merge_group(g, per_trial, k)
    assert merged.same_as(d3)  # merged on the device == prach_dist_merge of the per-trial results
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_dist(cfgs, 2048, groups=[0] * 39 + [3], ngroups=3)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:
        eng.run_trials_dist(cfgs, 2048, ngroups=39)
    assert ei.value.status == -1


def undisturbed_then(pkg, cfgs, bins, disturb, width=1):
    """The distributions of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, d = run_checked(pkg, e, cfgs, bins, width, groups=[k % 2 for k in range(len(cfgs))] if len(cfgs) > 1 else None)
            out.append((d, e.timing()))
        finally:
            e.close()
    (d0, t0), (d1, t1) = out
    assert d1.same_as(d0) and int(d1.trials.sum()) == len(cfgs)
    return t0, t1


def test_counted_once_calendar_rerun(pkg):
    cases = [(3000, {}), (8000, dict(nGrantUL=3)), (12000, dict(nGrantUL=2))]  # the shapes of test_calendar_cap_rerun_is_exact
    cfgs = [pkg.make_cfg(n, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s, **kw) for s in (0, 1) for n, kw in cases]
    t0, t1 = undisturbed_then(pkg, cfgs, 4096, lambda e: e.set("calendar_cap", 64))
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1.launches > t0.launches


def test_counted_once_mem_budget_split(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(8) for v in (0, 1) for n in (3000, 6000)]
    t0, t1 = undisturbed_then(pkg, cfgs, 4096, lambda e: e.set("mem_budget_mb", 64))
    assert t1.launches >= 2 and t1.launches > t0.launches


def test_counted_once_noma_ambiguity_rerun(pkg):
    for rng in (pkg.RNG_PHILOX, pkg.RNG_GLIBC):
        cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_NOMA_C, rng_mode=rng, seed=s) for n, s in ((2000, 1), (1000, 2))]
        t0, t1 = undisturbed_then(pkg, cfgs, 4096, lambda e: e.set("noma_ambiguity_test", 1))
        assert t1.fallback_trials >= 1


def test_counted_once_noma_glibc_window_retry(pkg):
    """NOMA.c in the reference's stream: a trial whose first window runs out (test_noma.py: RETRY_CASE) next to an ordinary one, two groups, in the
    single-launch form, slot by slot, and rerun slot by slot after the test hook — each trial is given a job by the run that finished it."""
    cfgs = [pkg.make_cfg(300, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC, seed=3, cellRadius=35.01),
            pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC, seed=4)]
    dists = []
    for key in (None, "noma_host_activation", "noma_ambiguity_test"):
        e = pkg.Engine(0)
        try:
            if key:
                e.set(key, 1)
            res, _, d = run_checked(pkg, e, cfgs, 4096, groups=[0, 1])  # (same_as dist_from_logs of the logs of the same call)
            assert e.timing().dist_ms > 0 and res[0].draws == 566735
        finally:
            e.close()
        assert int(d.trials.sum()) == 2 and d.trials.tolist() == [1, 1]
        dists.append(d)
    assert dists[1].same_as(dists[0]) and dists[2].same_as(dists[0])


def test_counted_once_stream_retry(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_GLIBC, seed=s) for n, v, s in ((5000, 0, 1), (5000, 1, 2), (20000, 1, 3))]
    t0, t1 = undisturbed_then(pkg, cfgs, 4096, lambda e: e.set("stream_factor", 1))
    assert t1.launches > t0.launches  # (a window of one draw per UE runs out: the trials are run again with a larger one)


def test_counted_once_resident_hook(pkg):
    cfgs = [pkg.make_cfg(20000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3)]  # the shapes of test_cluster_residency_is_explicit

    def narrow(e):
        e.set("cluster", 16)
        e.set("resident", 30)
    t0, t1 = undisturbed_then(pkg, cfgs, 4096, narrow)
    assert t1.resident_limit == 30 and t1.cluster_size == 8


def test_truncated_trial_counts_finished_ues_only(pkg, ob, eng):
    for rng in (pkg.RNG_GLIBC, pkg.RNG_PHILOX):
        cfg = pkg.make_cfg(8000, variant=1, rng_mode=rng, seed=9, max_steps=2500)
        res, logs, d = run_checked(pkg, eng, [cfg], 4096)
        ores, oues = ob.run_trial(ob.make_cfg(8000, variant=1, max_steps=2500), ob.Rng(rng, 9))
        assert d.same_as(bincount_dist(pkg, [as_array(oues)], 4096, 1, [0], 1))
        assert 0 < int(d.success[0]) == ores.nSuccessUE < 8000 and int(d.delay_sum[0]) == ores.sumTimer
        assert (as_array(logs[0])[:, FLAG] != 1).sum() == 8000 - ores.nSuccessUE


def test_isolation_from_plain_run_trials(pkg, eng):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s) for n, v, r, s in ((3000, 0, 1, 1), (5000, 1, 1, 2), (4000, 1, 0, 3))]
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().dist_ms == 0
    res1, logs1, _ = eng.run_trials_dist(cfgs, 512, 2, want_logs=True)
    assert eng.timing().dist_ms > 0
    res2, logs2 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().dist_ms == 0
    for res, logs in ((res1, logs1), (res2, logs2)):
        assert [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert all(bytes(a) == bytes(b) for a, b in zip(logs, logs0))
    _, nologs, d = eng.run_trials_dist(cfgs, 512, 2)  # without logs: the same distributions
    assert nologs == [None] * 3 and d.same_as(pkg.dist_from_logs(logs0, 512, 2))


@pytest.mark.parametrize("workers", [1, 4])
def test_cli_cdf_equals_the_logs(pkg, eng, tmp_path, workers):
    """prach_sim --cdf with --logs 0 on a shortened sweep, three seeds per point merged — and the same from four forked workers on one device."""
    out = tmp_path / "cdf.csv"
    cmd = [pkg.CLI_PATH, "--program", "beta", "-t", "3", "--rng", "philox", "--logs", "0", "--sweep", "2000:6000:2000", "--out", str(tmp_path), "--cdf", str(out),
           "--cdf-bins", "2048"]
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [2000, 4000, 6000]
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in points]
    _, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.dist_from_logs(logs, 2048, 1, groups=[k % 3 for k in range(9)], ngroups=3)
    assert out.read_bytes() == pkg.dist_csv(exp, labels=points) and len(out.read_bytes()) > 1000
