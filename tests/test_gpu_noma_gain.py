"""prach_run_trials_noma_gain on the GPU: the level pre-pass and prach::noma_gain_kernel, reducing the log records prach::noma_kernel leaves on the device and
the launch's own activation table, equal the host definition (noma_gain_from_logs: the host libm's levels) integer for integer — on twenty-four seeds of 300 and
of 3000 UEs in groups of several shapes under both schemes, with the table built by the device and by the host, under every cluster size, under a memory budget
that splits the call and under the NOMA_AMBIGUOUS rerun (a trial counts once), around the tile size and on the all-served early exit; results and logs are those
of plain prach_run_trials; the timing fields, the refusals, and prach_sim --census-gain against noma_gain_csv.  In every test on real trials the host resolves
fewer than 1 % of the arrived UEs (tests/test_noma_gain_cpu.py checks the seeds against the band on the CPU): the device path is what is being compared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_gain_ref as G  # noqa: E402
from test_noma_gain_cpu import GPU_SEEDS_300, GPU_SEEDS_3000  # noqa: E402

pytestmark = pytest.mark.gpu

SPEC = (65, 200, -16200)


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def noma_cfg(pkg, nUE, seed, **kw):
    return pkg.make_cfg(nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=seed, **kw)


def host_of(pkg, cfgs, res, logs, spec=SPEC, **kw):
    return pkg.noma_gain_from_logs(cfgs, [r.steps for r in res], logs, *spec, **kw)


def equal(gn, host):
    assert gn.same_as(host), G.same(gn, host)
    assert G.identity(gn)


def device_path(eng, gn):
    """The condition of every test on real trials: the host resolved fewer than 1 % of the arrived UEs."""
    arrived = int((gn.scalars["served"] + gn.scalars["dropped"] + gn.scalars["pending"]).sum())
    tm = eng.timing()
    assert arrived > 0 and tm.noma_gain_host_ues < 0.01 * arrived and tm.noma_gain_pad == 0, (tm.noma_gain_host_ues, arrived)
    return tm


@pytest.mark.parametrize("nue,seeds", [(300, GPU_SEEDS_300), (3000, GPU_SEEDS_3000)], ids=["300ues", "3000ues"])
def test_twenty_four_seeds_in_groups_of_several_shapes(pkg, eng, nue, seeds):
    cfgs = [noma_cfg(pkg, nue, s) for s in seeds]
    res, logs, per = eng.run_trials_noma_gain(cfgs, want_logs=True)  # one group per trial
    assert all(r.status == 0 for r in res) and len(cfgs) == 24
    equal(per, host_of(pkg, cfgs, res, logs))
    device_path(eng, per)
    assert (per.scalars["served"] > 0).all() and (per.scalars["below"] == 0).all() and (per.scalars["above"] == 0).all() and (per.scalars["undefined"] == 0).all()
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)  # results and logs are those of plain prach_run_trials
    assert [bytes(r) for r in res0] == [bytes(r) for r in res] and [bytes(l) for l in logs0] == [bytes(l) for l in logs]
    shapes = [([0] * 24, 1, SPEC), ([k % 5 for k in range(24)], 7, SPEC), (np.random.default_rng(3).permutation(24).tolist(), 24, (6, 1000, -12000)),
              ([k // 12 for k in range(24)], 2, (600, 25, -16200)), ([k % 3 for k in range(24)], 3, (4096, 4, -16384))]  # groups 5 and 6 of the second have no trial
    for scheme in (0, 1):
        eng.set("timeline_scheme", scheme)
        for groups, ng, spec in shapes:
            want = host_of(pkg, cfgs, res, logs, spec, groups=groups, ngroups=ng)
            for logs_wanted in ((False, [3]) if ng == 7 else (False,)):
                r2, l2, gn = eng.run_trials_noma_gain(cfgs, *spec, groups=groups, ngroups=ng, want_logs=logs_wanted)
                equal(gn, want)
                device_path(eng, gn)
                assert [bytes(r) for r in r2] == [bytes(r) for r in res] and all(l is None or bytes(l) == bytes(logs[k]) for k, l in enumerate(l2))
            if ng == 7:
                assert gn.scalars["level_max"][5:].tolist() == [-1, -1] and gn.scalars["defined"][5:].tolist() == [0, 0] and not gn.series[:, 5:].any()


def same_under(pkg, cfgs, *setups, spec=SPEC):
    """The same grouped call on one fresh engine per setup (None: as it is; else a function that sets options); every setup's profile equals the first's."""
    out = []
    for fn in setups:
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            res, _, gn = e.run_trials_noma_gain(cfgs, *spec, groups=[k % 2 for k in range(len(cfgs))], ngroups=2)
            assert all(r.status == 0 for r in res)
            out.append((gn, device_path(e, gn), res))
        finally:
            e.close()
    for gn, _, res in out[1:]:
        assert gn.same_as(out[0][0]), G.same(gn, out[0][0])
        assert int(gn.scalars["trials"].sum()) == len(cfgs) and int(gn.scalars["ues"].sum()) == sum(c.nUE for c in cfgs)
        assert [bytes(r) for r in res] == [bytes(r) for r in out[0][2]]
    return [t for _, t, _ in out]


def test_host_built_and_device_built_activation_tables_give_the_same_profile(pkg, eng):
    cfgs = [noma_cfg(pkg, n, s) for n in (300, 3000) for s in range(6)]
    t_dev, t_host = same_under(pkg, cfgs, lambda e: e.set("noma_host_activation", 0), lambda e: e.set("noma_host_activation", 1))
    assert t_dev.noma_gain_ms > 0 and t_host.noma_gain_ms > 0
    res, logs, gn = eng.run_trials_noma_gain(cfgs, want_logs=True)
    equal(gn, host_of(pkg, cfgs, res, logs))


def test_counted_once_under_the_ambiguity_rerun_and_a_split_call(pkg):
    """noma_ambiguity_test = 1: every gain sort counts as ambiguous, the trials are rerun with the host-built table; mem_budget_mb = 4 splits the call.  The
    records and levels of a discarded launch are never reduced: the profile is the undisturbed call's, every trial counted once."""
    cfgs = [noma_cfg(pkg, 3000, s, max_steps=2500) for s in range(16)]

    def split(e):
        e.set("mem_budget_mb", 4)

    def both(e):
        e.set("noma_ambiguity_test", 1)
        e.set("mem_budget_mb", 4)

    t0, ta, ts, tb = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1), split, both)
    assert t0.fallback_trials == 0 and ta.fallback_trials >= 1 and tb.fallback_trials >= 1
    assert ta.launches > t0.launches and ts.launches > t0.launches and tb.launches > ta.launches
    assert all(t.noma_gain_ms > 0 for t in (t0, ta, ts, tb))


@pytest.mark.parametrize("cluster", [1, 4, 32])  # the cluster sizes of the NOMA trial tests (tests/test_noma.py)
def test_cluster_sizes(pkg, eng, cluster):
    eng.set("cluster", cluster)
    cfgs = [noma_cfg(pkg, 3000, 21), noma_cfg(pkg, 300, 22)]
    res, logs, gn = eng.run_trials_noma_gain(cfgs, want_logs=True)
    assert all(r.status == 0 for r in res)
    equal(gn, host_of(pkg, cfgs, res, logs))
    device_path(eng, gn)
    assert [int(v) for v in gn.scalars["served"]] == [r.nSuccessUE for r in res]


def test_trials_around_the_tile_size_and_the_all_served_early_exit(pkg, eng):
    tile = pkg.noma_gain_tile_ues()
    cfgs = [noma_cfg(pkg, tile + d, 3 + d, max_steps=2500) for d in (-1, 0, 1)] + [noma_cfg(pkg, 100, 5, nGrantUL=30)]
    for scheme in (0, 1):
        eng.set("timeline_scheme", scheme)
        res, logs, gn = eng.run_trials_noma_gain(cfgs, want_logs=True)
        assert all(r.status == 0 for r in res) and res[3].nSuccessUE == 100 and int(res[3].steps) < 10000
        equal(gn, host_of(pkg, cfgs, res, logs))
        device_path(eng, gn)
        assert (gn.scalars["served"] > 0).all() and (gn.scalars["pending"][:3] > 0).all() and (gn.scalars["idle"][:3] > 0).all() and int(gn.scalars["pending"][3]) == 0


def test_timing_fields(pkg, eng):
    others = ("noma_timeline_ms", "noma_trace_ms", "noma_census_ms", "noma_columns_ms", "noma_summary_ms", "noma_pick_ms", "columns_ms", "pick_ms", "xtab_ms", "trace_ms",
              "summary_ms", "dist_ms", "timeline_ms", "sojourn_ms")
    cfgs = [noma_cfg(pkg, 3000, 1, max_steps=3000)]
    eng.run_trials(cfgs)
    assert eng.timing().noma_gain_ms == 0 and eng.timing().noma_gain_host_ues == 0
    eng.run_trials_noma_gain(cfgs)
    tm = eng.timing()
    assert tm.noma_gain_ms > 0 and all(getattr(tm, f) == 0 for f in others)
    eng.run_trials_noma_timeline(cfgs, 600, 5)
    tm = eng.timing()
    assert tm.noma_timeline_ms > 0 and tm.noma_gain_ms == 0 and tm.noma_gain_host_ues == 0
    eng.run_trials(cfgs)
    assert eng.timing().noma_gain_ms == 0


def test_refusals_leave_outputs_untouched_and_the_engine_goes_on(pkg, eng):
    L = pkg.lib()
    good = [noma_cfg(pkg, 1000, 1, max_steps=2000), noma_cfg(pkg, 500, 2, max_steps=2000)]
    for bad_cfgs in ([good[0], pkg.make_cfg(1000, variant=0, rng_mode=pkg.RNG_PHILOX)], [good[0], pkg.make_cfg(1000, variant=1, rng_mode=pkg.RNG_PHILOX)],
                     [good[0], pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]):
        n = len(bad_cfgs)
        gn = pkg.NomaGain(n, 40, 300, -16200)
        gn.series[:] = 7
        hdr = (pkg.PrachNomaGain * n)()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        sp = gn.spec()
        assert L.prach_run_trials_noma_gain(eng._h, (pkg.PrachCfg * n)(*bad_cfgs), n, (pkg.PrachResult * n)(), None, C.byref(sp), None, hdr, gn._series()) == -2
        assert (gn.series == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)
    for bad in (dict(bins=0), dict(bins=pkg.NOMA_GAIN_MAX_BINS + 1), dict(bins=10, width=0), dict(bins=10, ngroups=3), dict(bins=10, groups=[0, 2], ngroups=2),
                dict(bins=10, ngroups=0, groups=[0, 0])):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_gain(good, **bad)
        assert ei.value.status == -1, bad
    sp = pkg.PrachNomaGainSpec(4096, 1, 0, 911, 0)  # 36 x 911 x 4096 words > 2^27: judged before any output is touched
    one = np.zeros(1, dtype=np.uint64)
    ptrs = (C.POINTER(C.c_uint64) * 6)(*[one.ctypes.data_as(C.POINTER(C.c_uint64))] * 6)
    hdr = (pkg.PrachNomaGain * 911)()
    assert L.prach_run_trials_noma_gain(eng._h, (pkg.PrachCfg * 2)(*good), 2, (pkg.PrachResult * 2)(), None, C.byref(sp), (C.c_int32 * 2)(0, 1), hdr, ptrs) == -2
    assert one[0] == 0
    res, logs, gn = eng.run_trials_noma_gain(good, want_logs=True)  # the engine goes on
    assert all(r.status == 0 for r in res) and int(gn.arrived.sum()) > 0
    equal(gn, host_of(pkg, good, res, logs))


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_census_gain_equals_the_binding(pkg, eng, tmp_path, workers):
    """prach_sim --program noma --census-gain on a two-point sweep, three seeds per point merged — and the same from two forked workers on one device."""
    out = tmp_path / "gain.csv"
    cmd = [pkg.CLI_PATH, "--program", "noma", "-t", "3", "--sweep", "300:3000:2700", "--out", str(tmp_path), "--census-gain", str(out)]
    spec = SPEC
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers), "--census-gain-bins", "12", "--census-gain-width", "1000", "--census-gain-lo", "-16000"]
        spec = (12, 1000, -16000)
    else:
        cmd += ["--gpus", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [300, 3000]
    cfgs = [noma_cfg(pkg, n, s) for s in range(3) for n in points]
    _, _, exp = eng.run_trials_noma_gain(cfgs, *spec, groups=[k % 2 for k in range(6)], ngroups=2)
    assert out.read_bytes() == pkg.noma_gain_csv(exp, labels=points) and len(out.read_bytes()) > 300
    if workers == 1:
        assert int(exp.scalars["below"].sum()) == int(exp.scalars["above"].sum()) == 0  # the default axis covers every gain a trial draws
