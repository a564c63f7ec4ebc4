"""prach_run_trials_xtab on the GPU: the outcome cross-tabulations prach::xtab_kernel reduces on the device equal, integer for integer,
prach_xtab_accumulate_logs of the per-UE logs the same call returns (`xtab_from_logs`), a numpy restatement over those logs and — where an oracle run is
cheap — the same restatement over the oracle's UEs: behind every Beta.c / RandomAccessWithNOMA kernel, at the tile edges and on both sides of the table size
that selects the kernel's path, under both schemes, under every rerun the engine knows (a trial counts once), through groups, through prach_sim --xtab and
sweep.py --xtab; and the literal censuses of the four trials of tests/test_xtab_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import timeline_ref as T  # noqa: E402
import xtab_ref as X  # noqa: E402
from kernel_matrix import BETA_CASES, ROWS  # noqa: E402

pytestmark = pytest.mark.gpu

DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0, xtab_scheme=1)
ROW_NAMES = ("batch_w8_philox", "batch_w16_philox", "batch_glibc", "lcluster4_philox", "lcluster4_glibc", "cluster_wide_glibc", "legacy_philox")
ALL = X.SERVED | X.UNSERVED | X.IDLE
CENSUS = (("arrival", 500, 20), ("state", 1, 7), ALL)           # the drivers' default over Beta traffic
AGES = (("arrival", 500, 20), ("age", 5, 2002), X.UNSERVED)     # how long the UEs left behind had been in the system, by when they arrived
# every field on an axis, every class choice, widths that do not divide, tables of per-wavefront copies, of one copy and past the window
SPECS = [CENSUS, AGES, (("one", 1, 1), ("state", 1, 7), ALL), (("failcount", 3, 10), ("ptc", 1, 255), X.UNSERVED), (("state", 1, 7), ("timer", 7, 300), X.SERVED | X.UNSERVED),
         (("sojourn", 50, 201), ("completion", 700, 15), X.SERVED), (("age", 1, 10006), ("one", 1, 1), X.IDLE | X.UNSERVED), (("ptc", 2, 3), ("failcount", 1, 2), X.UNSERVED | X.SERVED),
         (("one", 1, 1), ("one", 1, 1), X.IDLE), (("completion", 1, 65536), ("state", 2, 2), ALL), (("timer", 1, 400), ("arrival", 100, 90), X.SERVED)]


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def ends(res):
    return [min(r.steps, r.maxTime) for r in res]


def from_arrays(pkg, cfgs, arrays, E, spec, grp, ngroups):
    return X.numpy_xtab(pkg, arrays, [pkg.arrival_schedule(c)[0] for c in cfgs], [c.accessTime for c in cfgs], E, *spec, groups=grp, ngroups=ngroups)


def run_checked(pkg, eng, cfgs, spec, groups=None, ngroups=None):
    """One call with logs: the device's table equals xtab_from_logs and numpy on the logs of the same call, and the identities hold."""
    res, logs, x = eng.run_trials_xtab(cfgs, *spec, groups=groups, want_logs=True, ngroups=ngroups)
    assert all(r.status == 0 for r in res)
    grp = list(range(len(cfgs))) if groups is None else list(groups)
    host = pkg.xtab_from_logs(cfgs, [r.steps for r in res], logs, *spec, groups=grp, ngroups=x.ngroups)
    assert x.same_as(host), (spec, X.describe(x), X.describe(host))
    assert x.same_as(from_arrays(pkg, cfgs, [T.as_array(l) for l in logs], ends(res), spec, grp, x.ngroups)), spec
    sc = x.scalars
    assert (x.cells.sum(axis=(1, 2)).astype(np.int64) + sc["undefined"]).tolist() == sc["selected"].tolist() and sc["binned"].tolist() == x.cells.sum(axis=(1, 2)).tolist()
    assert int(sc["served"].sum()) == sum(r.nSuccessUE for r in res) and int(sc["idle"].sum()) == sum(c.nUE - r.activeCheck for c, r in zip(cfgs, res))
    assert int(sc["trials"].sum()) == len(cfgs) and int(sc["ues"].sum()) == sum(c.nUE for c in cfgs) == int((sc["idle"] + sc["served"] + sc["unserved"]).sum())
    return res, logs, x


def both_schemes(pkg, eng, cfgs, spec, groups=None, ngroups=None):
    """run_checked under xtab_scheme 0 (global atomics only) and 1 (a table that fits privatised in LDS): identical results."""
    eng.set("xtab_scheme", 0)
    _, _, x0 = run_checked(pkg, eng, cfgs, spec, groups, ngroups)
    eng.set("xtab_scheme", 1)
    res, logs, x1 = run_checked(pkg, eng, cfgs, spec, groups, ngroups)
    assert x1.same_as(x0)
    return res, logs, x1


_oracle = {}


def oracle_array(ob, c):
    key = bytes(c)
    if key not in _oracle:
        res, ues = ob.run_trial(T.oracle_cfg(ob, c), ob.Rng(c.rng_mode, c.seed))
        _oracle[key] = (res, T.as_array(ues).copy())
    return _oracle[key]


def equals_oracle(pkg, ob, cfgs, x, spec):
    exp = [oracle_array(ob, c) for c in cfgs]
    assert x.same_as(from_arrays(pkg, cfgs, [a for _, a in exp], ends([r for r, _ in exp]), spec, list(range(len(cfgs))), len(cfgs))), spec
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
        res, logs, x = both_schemes(pkg, eng, cfgs, CENSUS)
        tm = eng.timing()
        assert tm.xtab_ms > 0 and tm.dist_ms == 0 and tm.timeline_ms == 0 and tm.sojourn_ms == 0 and tm.trace_ms == 0 and tm.summary_ms == 0
        ores = equals_oracle(pkg, ob, cfgs, x, CENSUS)
        assert x.scalars["served"].tolist() == [r.nSuccessUE for r in ores] and x.scalars["idle"].tolist() == [c.nUE - r.activeCheck for c, r in zip(cfgs, ores)]
        if tm.fallback_trials == 0:
            assert {k: getattr(tm, k) for k in row["pin"]} == row["pin"] and tm.trial_kernel_reruns == 0
            counted += len(call)
        _, _, x = run_checked(pkg, eng, cfgs, SPECS[3])  # the words of a record the census does not read
        equals_oracle(pkg, ob, cfgs, x, SPECS[3])
    assert counted >= 1, "no call of this row stayed on its kernel"


def test_every_field_and_class_on_mixed_sizes_in_one_call(pkg, ob, eng):
    tile = pkg.xtab_tile_ues()
    sizes = [1, 37, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 4099]  # (trials of different nUE side by side: every job boundary is a workgroup's)
    cfgs = [pkg.make_cfg(n, variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k, maxMsg2TxCount=3, nGrantUL=4) for k, n in enumerate(sizes)]
    cfgs[5].max_steps = 3000  # one trial cut short: idle UEs, and an E below maxTime
    for spec in SPECS:
        res, _, x = both_schemes(pkg, eng, cfgs, spec)
    assert res[5].steps == 3000 and int(x.scalars["trials"].sum()) == len(sizes)
    _, _, x = both_schemes(pkg, eng, cfgs, CENSUS, groups=[0, 1, 0, 1, 0, 1, 2, 2, 2, 0])  # grouped trials of mixed size, the cut one among them
    assert int(x.scalars["idle"][1]) > 0 and x.scalars["trials"].tolist() == [4, 3, 3]
    equals_oracle(pkg, ob, cfgs[:6], eng.run_trials_xtab(cfgs[:6], *AGES)[2], AGES)


def test_both_sides_of_the_window(pkg, ob, eng):
    """A table of exactly xtab_window_words() cells is privatised in LDS, one cell more goes to global memory; a 1 x 1 table; tables small enough for one
    copy per wavefront and just too large for it."""
    words = pkg.xtab_window_words()
    c = pkg.make_cfg(8193, variant=1, rng_mode=pkg.RNG_PHILOX, seed=22, nGrantUL=4)
    assert words == 4096 * 7 and words + 1 == 53 * 541
    for spec in ((("arrival", 3, 4095), ("state", 1, 6), ALL), (("age", 200, 52), ("timer", 1, 540), X.SERVED | X.UNSERVED), (("arrival", 10, 1023), ("one", 1, 1), ALL),
                 (("one", 1, 1), ("one", 1, 1), ALL), (("timer", 1, 1), ("ptc", 1, 1), X.UNSERVED), (("arrival", 20, 511), ("state", 1, 1), ALL), (("arrival", 20, 512), ("state", 1, 1), ALL),
                 (("sojourn", 1, 65536), ("arrival", 5000, 2), X.SERVED)):
        _, _, x = both_schemes(pkg, eng, [c], spec)
        equals_oracle(pkg, ob, [c], x, spec)
        cells = (spec[0][2] + 1) * (spec[1][2] + 1)
        assert cells in (words, words + 1, 2048, 4, 1024, 1026, 65537 * 3)
    assert int(x.cells[0, :, 2].sum()) == 0 and int(x.cells[0, 65536].sum()) == 0 and int(x.scalars["binned"][0]) == 5141


CENSUS_TRIALS = [  # (nUE, overrides, UEs per state, the largest failCount): tests/test_xtab_cpu.py computes the same on the oracle
    (20000, dict(variant=1, seed=7, maxMsg2TxCount=3), [0, 17782, 1563, 623, 22, 10, 0], 122),
    (8193, dict(variant=0, seed=21, nGrantUL=4, max_steps=4000), [3992, 1870, 1588, 734, 6, 3, 0], None),
    (8193, dict(variant=0, seed=21, nGrantUL=4), [0, 5121, 2160, 904, 6, 2, 0], None),
    (8193, dict(variant=1, seed=22, nGrantUL=4), [0, 5141, 2089, 955, 6, 2, 0], 51)]


def test_the_four_census_trials(pkg, ob, eng):
    cfgs = [pkg.make_cfg(n, rng_mode=pkg.RNG_PHILOX, nPreamble=54, backoff=20, maxRarWindow=6, accessTime=5, **dict(dict(maxMsg2TxCount=9), **kw)) for n, kw, _, _ in CENSUS_TRIALS]
    spec = (("one", 1, 1), ("state", 1, 7), ALL)
    _, _, x = both_schemes(pkg, eng, cfgs, spec)
    equals_oracle(pkg, ob, cfgs, x, spec)
    assert [x.cells[k, 0, :7].tolist() for k in range(4)] == [s for _, _, s, _ in CENSUS_TRIALS] and not x.cells[:, 1].any() and not x.cells[:, 0, 7].any()
    _, _, f = both_schemes(pkg, eng, cfgs, (("one", 1, 1), ("failcount", 1, 255), X.UNSERVED | X.SERVED))
    assert [int(f.scalars["col_max"][k]) for k in (0, 3)] == [122, 51] and f.scalars["col_max"].tolist()[1:3] == [0, 0]
    _, _, a = both_schemes(pkg, eng, cfgs, AGES)
    equals_oracle(pkg, ob, cfgs, a, AGES)
    assert a.scalars["selected"].tolist() == [2218, 2331, 3072, 3052] and a.scalars["undefined"].tolist() == [0, 0, 0, 0]


def undisturbed_then(pkg, cfgs, disturb):
    """The table of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, x = run_checked(pkg, e, cfgs, CENSUS, groups=[k % 2 for k in range(len(cfgs))] if len(cfgs) > 1 else None)
            out.append((x, e.timing()))
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
    assert t1.launches >= 2 and t1.launches > t0.launches


def test_counted_once_capacity_fallback(pkg):
    """A 4-workgroup lean cluster whose per-subframe capacity the trial exceeds: rerun exactly on the next kernel of the ladder (kernel_matrix.LEAVES)."""
    n, kw = next((n, kw) for name, n, kw in BETA_CASES if name == "corner_5000")
    cfgs = [pkg.make_cfg(n, variant=1, rng_mode=pkg.RNG_PHILOX, seed=3, **kw)]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("cluster", 4))
    assert t1.fallback_trials >= 1 and t1.launches > t0.launches


def test_counted_once_stream_retry(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_GLIBC, seed=s) for n, v, s in ((5000, 0, 1), (5000, 1, 2), (20000, 1, 3))]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("stream_factor", 1))
    assert t1.launches > t0.launches  # (a window of one draw per UE runs out: the trials are run again with a larger one)


def test_groups_and_refusals(pkg, eng):
    rng = np.random.default_rng(3)
    cfgs = [pkg.make_cfg(int(n), variant=k % 2, rng_mode=pkg.RNG_PHILOX, seed=k, nGrantUL=3) for k, n in enumerate(rng.integers(500, 3000, 40))]  # unequal nUE in every group
    groups = rng.permutation(np.arange(40) % 3).tolist()
    _, _, x3 = both_schemes(pkg, eng, cfgs, CENSUS, groups=groups)
    _, _, x5 = run_checked(pkg, eng, cfgs, CENSUS, groups=[g if g < 2 else 4 for g in groups], ngroups=6)  # groups 2, 3 and 5 have no trial
    for g in (2, 3, 5):
        assert int(x5.scalars["row_max"][g]) == int(x5.scalars["col_max"][g]) == -1 and not x5.cells[g].any()
        assert [int(x5.scalars[f][g]) for f in pkg.XTAB_FIELDS[:-2]] == [0] * 10
    _, _, per_trial = run_checked(pkg, eng, cfgs, CENSUS)  # identity grouping, a second call
    merged = pkg.Xtab(3, *CENSUS)
    for k, g in enumerate(groups):
        merged.merge_group(g, per_trial, k)
    assert merged.same_as(x3)  # merged on the device == prach_xtab_merge of the per-trial results
    for bad in (dict(groups=[0] * 39 + [3], ngroups=3), dict(ngroups=39), dict(who=0), dict(who=8), dict(rows=("arrival", 0, 20)), dict(cols=("state", 1, 65537)), dict(rows=(9, 1, 1)),
                dict(cols=(-1, 1, 1))):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_xtab(cfgs, **bad)
        assert ei.value.status == -1, bad
    with pytest.raises(pkg.PrachError) as ei:  # 40 x 2048 x 2048 words > 2^27
        eng.run_trials_xtab(cfgs, ("arrival", 1, 2047), ("age", 1, 2047))
    assert ei.value.status == -2
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c: refused before anything is launched
        eng.run_trials_xtab(cfgs[:2] + [pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1)])
    assert ei.value.status == -2


def test_isolation_and_alternation_with_the_other_reductions(pkg, eng):
    """The xtab shares the device buffer, the job table and the events of the other kinds: they alternate on one engine, a small buffer after a large one.
    Plain results and logs are what they are without it; every other *_ms stays 0 in an xtab call and xtab_ms is 0 in every other call."""
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s) for n, v, r, s in ((3000, 0, 1, 1), (8193, 1, 1, 2), (4000, 1, 0, 3))]
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().xtab_ms == 0
    exp = pkg.xtab_from_logs(cfgs, [r.steps for r in res0], logs0, *CENSUS)
    for step in ("xtab", "sojourn", "xtab_big", "timeline", "xtab_nologs", "dist", "xtab_one"):
        tm_other = None
        if step == "sojourn":
            res, logs, _ = eng.run_trials_sojourn(cfgs, 21, 500, 2002, 5, want_logs=True)
            tm_other = eng.timing().sojourn_ms
        elif step == "timeline":
            res, logs, _ = eng.run_trials_timeline(cfgs, 2002, 5, want_logs=True)
            tm_other = eng.timing().timeline_ms
        elif step == "dist":
            res, logs, _ = eng.run_trials_dist(cfgs, 16, 1, want_logs=True)
            tm_other = eng.timing().dist_ms
        elif step == "xtab_nologs":
            res, logs, x = eng.run_trials_xtab(cfgs, *CENSUS, want_logs=[1])
            assert logs[0] is None and logs[2] is None and bytes(logs[1]) == bytes(logs0[1]) and x.same_as(exp)
            logs = logs0
        else:
            spec = dict(xtab=CENSUS, xtab_big=(("age", 1, 10006), ("state", 1, 7), ALL), xtab_one=(("one", 1, 1), ("one", 1, 1), ALL))[step]
            res, logs, x = eng.run_trials_xtab(cfgs, *spec, want_logs=True)
            assert x.same_as(pkg.xtab_from_logs(cfgs, [r.steps for r in res0], logs0, *spec))
        tm = eng.timing()
        if tm_other is None:
            assert tm.xtab_ms > 0 and (tm.dist_ms, tm.timeline_ms, tm.sojourn_ms, tm.trace_ms, tm.summary_ms) == (0, 0, 0, 0, 0)
        else:
            assert tm_other > 0 and tm.xtab_ms == 0
        assert [bytes(r) for r in res] == [bytes(r) for r in res0] and all(bytes(a) == bytes(b) for a, b in zip(logs, logs0))


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_xtab_equals_the_logs(pkg, eng, tmp_path, workers):
    """prach_sim --xtab with --logs 0 on a shortened sweep, three seeds per point merged — and the same from two forked workers on one device."""
    out = tmp_path / "xtab.csv"
    cmd = [pkg.CLI_PATH, "--program", "beta", "-t", "3", "--rng", "philox", "--logs", "0", "--sweep", "2000:6000:2000", "--out", str(tmp_path), "--xtab", str(out)]
    spec = CENSUS
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers), "--xtab-rows", "arrival:700", "--xtab-cols", "age:250", "--xtab-who", "arrived"]
        spec = (("arrival", 700, 15), ("age", 250, 41), X.SERVED | X.UNSERVED)
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [2000, 4000, 6000]
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in points]
    res, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.xtab_from_logs(cfgs, [r.steps for r in res], logs, *spec, groups=[k % 3 for k in range(9)], ngroups=3)
    assert out.read_bytes() == pkg.xtab_csv(exp, labels=points) and len(out.read_bytes()) > 400
    for other in ("--cdf", "--timeline", "--sojourn", "--ci", "--trace"):
        bad = subprocess.run(cmd + [other, str(tmp_path / "other.csv")], capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--xtab cannot be combined" in bad.stdout
    bad = subprocess.run([pkg.CLI_PATH, "--program", "noma", "--xtab", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--xtab needs --program beta or withnoma" in bad.stdout


def test_sweep_driver_xtab_two_ranks(pkg, eng, tmp_path):
    """sweep.py --xtab with 2 ranks rehearsed on one GPU (gloo): every rank's groups merged by allreduce_xtab, rank 0 writes the CSV of the logs."""
    out = tmp_path / "xtab.csv"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29543",
           os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--times", "3", "--sweep", "2000:6000:2000", "--out", str(tmp_path), "--backend", "gloo",
           "--same-device", "--xtab", str(out), "--xtab-rows", "state", "--xtab-cols", "timer:3:50", "--xtab-who", "arrived"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    points = [2000, 4000, 6000]
    cfgs = [pkg.make_cfg(n, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(3) for n in points]
    res, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.xtab_from_logs(cfgs, [r.steps for r in res], logs, ("state", 1, 7), ("timer", 3, 50), X.SERVED | X.UNSERVED, groups=[k % 3 for k in range(9)], ngroups=3)
    assert out.read_bytes() == pkg.xtab_csv(exp, labels=points) and len(out.read_bytes()) > 400
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--xtab", str(out), "--trace", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--xtab cannot be combined" in bad.stderr
