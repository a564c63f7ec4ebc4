"""Host side of NOMA.c's near-far profile (include/prach.h, prach_noma_gain_*): the gain level; the definition prach::noma_gain_kernel must equal, against the
numpy restatement of tests/tools/noma_gain_ref.py over the ORACLE's UEs (300 and 3000 UEs, an early exit, a run to maxTime, cell-wide grouping); the identity,
from_logs against from_levels, the merge in two orders, the CSV bytes of a hand-made group, the structs and the prach_timing placements against a compiled C
program, every argument and refusal that needs no device, the CLI's messages, the kernels' symbols, the share of UEs the device pre-pass would hand to the host
on the seeds the GPU tests use, and a sanitised stand-alone run of the new host functions (tests/tools/noma_gain_host_check.c).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import noma_census_ref as N  # noqa: E402
import noma_gain_cases as GC  # noqa: E402
import noma_gain_ref as G  # noqa: E402

# (nUE, seed, product kwargs): NOMA.c's 300 and 3000 UEs to maxTime, a trial that exits early (every UE served), the cell-wide grouping, a cut run
CASES = [(300, 0, {}), (3000, 0, {}), (100, 5, dict(nGrantUL=30)), (2000, 9, dict(flags=2)), (2000, 6, dict(nGrantUL=1, maxMsg2TxCount=3, max_steps=4325))]
# (bins, width, lo): the default axis; a coarse one that leaves UEs below and above; one bin; 4096 bins of 4 levels
SPECS = [(65, 200, -16200), (6, 1000, -12000), (1, 20000, -20000), (4096, 4, -16384)]
ERR_ARG, ERR_UNSUPPORTED = -1, -2  # PRACH_ERR_ARG, PRACH_ERR_UNSUPPORTED (include/prach.h)
# the seeds of the engine tests on the GPU (tests/test_gpu_noma_gain.py): checked here to stay clear of the pre-pass's band
GPU_SEEDS_300, GPU_SEEDS_3000 = tuple(range(24)), tuple(range(24))


def product_cfg(pkg, n, seed, kw):
    return pkg.make_cfg(n, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=seed, **kw)


def oracle_trial(ob, n, seed, kw):
    okw = dict(kw)
    if "maxMsg2TxCount" in okw:
        okw["maxMsg1ReTx"] = okw.pop("maxMsg2TxCount")
    if "flags" in okw:
        okw["nonsector"] = 1 if okw.pop("flags") & 2 else 0
    res, ues = ob.noma_run_trial(ob.make_noma_cfg(n, **okw), ob.Rng(ob.RNG_PHILOX, seed))
    return res, N.as_array(ues)


@pytest.fixture(scope="module")
def trials(pkg, ob):
    """(product cfg, oracle result, oracle UEs as int32 [nUE, 16], schedule, E, host levels) per case, computed once."""
    out = []
    for n, seed, kw in CASES:
        c = product_cfg(pkg, n, seed, kw)
        res, a = oracle_trial(ob, n, seed, kw)
        out.append((c, res, a, pkg.arrival_schedule(c)[0], min(int(res.steps), 10000), pkg.noma_gain_levels(c)))
    return out


def ref_of(trial, bins, width, lo):
    c, res, a, sched, E, lv = trial
    return G.profile([a], [sched], [c.accessTime], [E], [lv], bins, width, lo)


def test_gain_level_at_integers_halves_negatives_and_no_level(pkg):
    lvl = pkg.noma_gain_level
    for k in (0, 1, -1, 7, -7, 16118, -16119, 2 ** 20, -(2 ** 20), 2 ** 30 - 1024, -(2 ** 30 - 1024)):
        assert lvl(k / 1024.0 * 1.024) == int(np.floor(np.float64(1000.0) * np.float64(k / 1024.0 * 1.024)))
        assert abs(125 * k) >= 2 ** 30 or lvl(k / 8.0) == 125 * k  # 1000 x (k / 8) is exact: the level of an exact integer product is that integer
    assert [lvl(v) for v in (0.0, 0.001, -0.001, 0.0005, -0.0005, 1.0, -1.0, -3.3505, -16.1181, 0.9999999)] == [0, 1, -1, 0, -1, 1000, -1000, -3351, -16119, 999]
    assert lvl(-0.0) == 0 and lvl(5e-324) == 0 and lvl(-5e-324) == -1  # floor, not truncation
    for v in (float("inf"), float("-inf"), float("nan"), 2.0 ** 30 / 1000.0 * 1.0000001, -(2.0 ** 30) / 1000.0 * 1.0000001, 1e300, -1e300):
        assert lvl(v) == pkg.NOMA_GAIN_NO_LEVEL == G.NO_LEVEL == -2 ** 31
    assert lvl(1073741.5) == int(np.floor(np.float64(1000.0) * np.float64(1073741.5))) and lvl(-1073741.5) == int(np.floor(np.float64(-1000.0) * np.float64(1073741.5)))  # just inside 2^30
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(-17, -3, 2000), rng.uniform(-2e6, 2e6, 2000), rng.integers(-20000, 20000, 2000) / 1000.0])
    assert [lvl(float(x)) for x in xs] == G.level_of(xs).tolist()


def test_levels_of_a_cfg_against_numpy_on_the_activation_table(pkg, trials):
    for c, res, a, sched, E, lv in trials[:2]:
        lg = pkg.noma_activation_table(c)[3]
        assert lv.dtype == np.int32 and np.array_equal(lv, G.level_of(lg))
        assert -16200 < lv.min() and lv.max() < -3300  # a trial's range: gain >= 1e-7, and at most what the smallest path loss allows
    for bad, status in ((pkg.make_cfg(300, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC), ERR_UNSUPPORTED), (pkg.make_cfg(300, variant=0, rng_mode=pkg.RNG_PHILOX), ERR_UNSUPPORTED)):
        with pytest.raises(pkg.PrachError) as ei:
            pkg.noma_gain_levels(bad)
        assert ei.value.status == status


def test_inputs_populate_what_the_comparison_needs(trials):
    """Asserted on the oracle's side, before anything is compared."""
    c, res, a, sched, E, lv = trials[4]
    assert set(np.unique(N.classes(a))) == {N.SERVED, N.PENDING, N.IDLE, N.DROPPED}
    full = ref_of(trials[1], 65, 200, -16200)
    assert all(full["series"][G.ARRIVED, 0, s].sum() > 0 and full["series"][G.SERVED, 0, s].sum() > 0 for s in range(6))
    assert int(full["scalars"]["below"][0]) == int(full["scalars"]["above"][0]) == 0  # the default axis covers every gain a trial draws
    coarse = ref_of(trials[1], 6, 1000, -12000)
    assert int(coarse["scalars"]["below"][0]) > 0 and int(coarse["scalars"]["above"][0]) > 0
    assert trials[2][1].nSuccessUE == 100 and int(trials[2][1].steps) < 10000 and int(trials[1][1].steps) == 10000  # an early exit; a run to maxTime


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s[0]}x{s[1]}from{s[2]}")
def test_definition_equals_numpy_on_oracle_ues(pkg, trials, spec):
    for trial in trials:
        c, res, a, sched, E, lv = trial
        host = pkg.noma_gain_from_logs([c], [res.steps], [a], *spec)
        ref = ref_of(trial, *spec)
        assert G.same(host, ref) is None, (c.nUE, c.seed, spec, G.same(host, ref))
        assert G.identity(host) and G.identity(ref)  # (with and without PRACH_FLAG_NOMA_NONSECTOR: CASES has both)
        given = pkg.noma_gain_from_levels([c], [res.steps], [a], [lv], *spec)
        assert given.same_as(host)  # from_logs == from_levels(host levels)
        sc = {f: int(v[0]) for f, v in host.scalars.items()}
        assert sc["ues"] == c.nUE and sc["served"] == res.nSuccessUE and sc["idle"] == c.nUE - res.activeCheck and sc["dropped"] == res.raFailedUEs and sc["undefined"] == 0
        assert sc["level_max"] == int(lv[N.classes(a) != N.IDLE].max()) and sc["neg_level_max"] == -int(lv[N.classes(a) != N.IDLE].min())
        assert int(host.sojourn_sum.sum()) <= sc["sojourn_sum"] and int(host.lost_sum.sum()) <= sc["lost_sum"] <= sc["sojourn_sum"] and int(host.ptc_sum.sum()) <= sc["ptc_sum"]
        if spec == SPECS[0]:
            assert int(host.sojourn_sum.sum()) == sc["sojourn_sum"] and int(host.ptc_sum.sum()) == sc["ptc_sum"] and int(host.served.sum()) == sc["served"]
    assert (pkg.noma_gain_from_logs([trials[3][0]], [trials[3][1].steps], [trials[3][2]], *spec).arrived[0].sum(axis=1) > 0).all()  # non-sector: the UE's own sector, all six


def test_views_ratios_and_edges(pkg, trials):
    c, res, a, sched, E, lv = trials[1]
    gn = pkg.noma_gain_from_logs([c], [res.steps], [a])
    assert (gn.bins, gn.width, gn.lo) == (65, 200, -16200) and gn.arrived.shape == (1, 6, 65) and gn.arrived.base is gn.series and gn.ptc_sum.base is gn.series
    assert np.array_equal(gn.edges(), -16200 + 200 * np.arange(65)) and gn.edges()[-1] + 200 == -3200
    pend = gn.arrived.astype(np.int64) - gn.served.astype(np.int64) - gn.dropped.astype(np.int64)
    assert (pend >= 0).all() and int(pend.sum()) == int(gn.scalars["pending"][0]) > 0
    for sector in (None, 0, 5):
        arr, sv, dr = gn.named("arrived", 0, sector), gn.named("served", 0, sector), gn.named("dropped", 0, sector)
        sr, drr, ms, ml, mp = gn.served_ratio(0, sector), gn.dropped_ratio(0, sector), gn.mean_sojourn(0, sector), gn.mean_lost(0, sector), gn.mean_ptc(0, sector)
        arr_, sv_ = np.maximum(arr, 1), np.maximum(sv, 1)
        assert np.array_equal(np.isnan(sr), arr == 0) and np.array_equal(np.isnan(drr), arr == 0) and all(np.array_equal(np.isnan(m), sv == 0) for m in (ms, ml, mp))
        assert np.array_equal(sr[arr > 0], (sv / arr_)[arr > 0]) and np.array_equal(drr[arr > 0], (dr / arr_)[arr > 0])
        for m, name in ((ms, "sojourn_sum"), (ml, "lost_sum"), (mp, "ptc_sum")):
            assert np.array_equal(m[sv > 0], (gn.named(name, 0, sector) / sv_)[sv > 0])
        assert (mp[sv > 0] >= 0).all() and (mp[sv > 0] > 0).any() and (ml[sv > 0] <= ms[sv > 0]).all()


def test_groups_and_merge_are_order_free(pkg, trials):
    cfgs, steps, arrays, levels = [t[0] for t in trials], [t[1].steps for t in trials], [t[2] for t in trials], [t[5] for t in trials]
    groups = [k % 3 for k in range(len(trials))]
    grouped = pkg.noma_gain_from_logs(cfgs, steps, arrays, 7, 1000, -12000, groups=groups, ngroups=4)
    ref = G.profile(arrays, [t[3] for t in trials], [t[0].accessTime for t in trials], [t[4] for t in trials], levels, 7, 1000, -12000, groups=groups, ngroups=4)
    assert G.same(grouped, ref) is None and G.identity(grouped)
    assert int(grouped.scalars["level_max"][3]) == int(grouped.scalars["neg_level_max"][3]) == -1 and int(grouped.scalars["defined"][3]) == 0
    assert (grouped.scalars["level_max"][:3] < -1).all()  # a real maximum below the empty group's -1: the merge must not let the empty side win
    single = pkg.noma_gain_from_logs(cfgs, steps, arrays, 7, 1000, -12000)
    for order in (list(range(5)), list(reversed(range(5)))):
        m = pkg.NomaGain(4, 7, 1000, -12000)
        for k in order:
            m.merge_group(groups[k], single, k)
        assert m.same_as(grouped), order
    fresh = lambda k: pkg.noma_gain_from_logs([cfgs[k]], [steps[k]], [arrays[k]], 7, 1000, -12000)
    assert fresh(0).merge(fresh(3)).merge(fresh(4)).same_as(fresh(0).merge(fresh(3).merge(fresh(4))))
    e = pkg.NomaGain(1, 7, 1000, -12000)
    assert e.merge(pkg.NomaGain(1, 7, 1000, -12000)).same_as(pkg.NomaGain(1, 7, 1000, -12000)) and fresh(0).merge(e).same_as(fresh(0)) and e.merge(fresh(0)).same_as(fresh(0))
    with pytest.raises(ValueError):
        e.merge(pkg.NomaGain(1, 7, 1000, -12001))


def filled(pkg):
    a = pkg.NomaGain(1, 3, 100, -500)
    a.series[:, 0, 0, 0] = (4, 3, 1, 90, 60, 5)
    a.series[:, 0, 2, 0] = (1, 0, 0, 0, 0, 0)
    a.series[:, 0, 5, 2] = (9, 4, 0, 400, 40, 9)
    for f, v in zip(pkg.NOMA_GAIN_FIELDS, (1, 20, 3, 7, 1, 6, 1, 2, 0, 2, 490, 100, 14, 16, -250, 520)):
        a.scalars[f][0] = v
    b = pkg.NomaGain(1, 3, 100, -500)
    b.series[:, 0, 0, 0] = (2, 2, 0, 30, 0, 2)
    b.series[:, 0, 1, 1] = (6, 0, 2, 0, 0, 0)
    for f, v in zip(pkg.NOMA_GAIN_FIELDS, (2, 11, 0, 2, 2, 4, 0, 0, 3, 0, 30, 0, 2, 11, -10, 480)):
        b.scalars[f][0] = v
    return a, b


CSV = b"""p,arrived,all,below,2
p,arrived,0,-500,6
p,arrived,2,-500,1
p,arrived,all,-500,7
p,arrived,1,-400,6
p,arrived,all,-400,6
p,arrived,5,-300,9
p,arrived,all,-300,9
p,arrived,all,above,3
p,served,0,-500,5
p,served,all,-500,5
p,served,5,-300,4
p,served,all,-300,4
p,dropped,0,-500,1
p,dropped,all,-500,1
p,dropped,1,-400,2
p,dropped,all,-400,2
p,sojourn_sum,0,-500,120
p,sojourn_sum,all,-500,120
p,sojourn_sum,5,-300,400
p,sojourn_sum,all,-300,400
p,lost_sum,0,-500,60
p,lost_sum,all,-500,60
p,lost_sum,5,-300,40
p,lost_sum,all,-300,40
p,ptc_sum,0,-500,7
p,ptc_sum,all,-500,7
p,ptc_sum,5,-300,9
p,ptc_sum,all,-300,9
"""


def test_merge_and_csv_against_a_literal_block(pkg):
    a, b = filled(pkg)
    ab, ba = filled(pkg)[0].merge(b), filled(pkg)[1].merge(a)
    assert ab.same_as(ba)
    assert [int(ab.scalars[f][0]) for f in pkg.NOMA_GAIN_FIELDS] == [3, 31, 3, 9, 3, 10, 1, 2, 3, 2, 520, 100, 16, 27, -10, 520]
    assert pkg.noma_gain_csv(ab, labels=["p"]) == CSV
    empty = pkg.NomaGain(2)
    assert pkg.noma_gain_csv(empty) == b"" and empty.scalars["level_max"].tolist() == [-1, -1] and empty.scalars["neg_level_max"].tolist() == [-1, -1]
    one = pkg.NomaGain(1, 3, 100, 2 ** 31 - 301)  # the last edge is formed in 64 bits
    one.series[0, 0, 2, 2] = 5
    assert pkg.noma_gain_csv(one, labels=["p"]) == b"p,arrived,2,2147483547,5\np,arrived,all,2147483547,5\n"


def test_struct_sizes_offsets_and_timing_placements(pkg, tmp_path):
    src = tmp_path / "sz.c"
    fields = list(pkg.NOMA_GAIN_FIELDS)
    sfields = ["bins", "width", "lo", "ngroups", "reserved"]
    tfields = ["noma_host_ues", "noma_gain_host_ues", "noma_gain_pad", "noma_gain_ms", "noma_timeline_ms", "noma_trace_ms", "sojourn_ms"]
    offs = ", ".join([f"offsetof(prach_noma_gain, {f})" for f in fields] + [f"offsetof(prach_noma_gain_spec, {f})" for f in sfields] + [f"offsetof(prach_timing, {f})" for f in tfields])
    src.write_text('#include "prach.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){long long v[] = {sizeof(prach_noma_gain), sizeof(prach_noma_gain_spec), sizeof(prach_timing), '
                   'PRACH_NOMA_GAIN_SERIES, PRACH_NOMA_GAIN_MAX_BINS, PRACH_NOMA_GAIN_NO_LEVEL, PRACH_NOMA_NFIELDS, ' + offs +
                   '}; for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf("%lld ", v[i]); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    S, Gs, TM = pkg.PrachNomaGainSpec, pkg.PrachNomaGain, pkg.PrachTiming
    assert got == [C.sizeof(Gs), C.sizeof(S), C.sizeof(TM), 6, pkg.NOMA_GAIN_MAX_BINS, pkg.NOMA_GAIN_NO_LEVEL, 13] + [getattr(Gs, f).offset for f in fields] + \
        [getattr(S, f).offset for f in sfields] + [getattr(TM, f).offset for f in tfields]
    assert C.sizeof(Gs) == 8 * 16 and C.sizeof(S) == 20 and fields[:2] == ["trials", "ues"] and fields[-2:] == ["level_max", "neg_level_max"]
    # prach_timing: noma_gain_host_ues and a pad in front of noma_gain_ms, that directly in front of noma_timeline_ms, which stays 8 in front of noma_trace_ms; sojourn_ms last
    assert TM.noma_gain_host_ues.offset + 4 == TM.noma_gain_pad.offset and TM.noma_gain_pad.offset + 4 == TM.noma_gain_ms.offset
    assert TM.noma_gain_ms.offset + 8 == TM.noma_timeline_ms.offset and TM.noma_timeline_ms.offset + 8 == TM.noma_trace_ms.offset
    assert TM._fields_[-1][0] == "sojourn_ms" and TM.sojourn_ms.offset + 8 == C.sizeof(TM)
    assert pkg.NOMA_GAIN_SERIES == G.SERIES and pkg.NOMA_GAIN_FIELDS == G.SCALARS and len(pkg.NOMA_FIELD_NAMES) == 13
    assert pkg.noma_gain_tile_ues() == pkg.timeline_tile_ues() == GC.TILE and pkg.noma_gain_lds_max_bins() == GC.LDS_MAX_BINS
    # the counters of the largest LDS size, the staged schedule range and the scalars leave room for two workgroups on a CU's 160 KiB of LDS; one bin more does not
    assert 2 * (4 * (2048 + 36 * pkg.noma_gain_lds_max_bins()) + 128) <= 160 * 1024 < 2 * (4 * (2048 + 36 * (pkg.noma_gain_lds_max_bins() + 1)) + 128)


def test_call_argument_and_refusal_matrix(pkg):
    """Spec, groups and variants are judged before the engine is looked at: with engine == NULL every refusal comes, nothing is written, and an acceptable call
    ends with PRACH_ERR_ARG for the missing engine."""
    L = pkg.lib()
    noma = lambda **kw: pkg.make_cfg(500, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1, **kw)

    def call(cfgs, bins=65, width=200, lo=-16200, ngroups=None, groups=None, reserved=0, null=None, n=None):
        n = len(cfgs) if n is None else n
        ng = len(cfgs) if ngroups is None else ngroups
        gn = pkg.NomaGain(max(ng, 1), min(max(bins, 1), 8), max(width, 1), lo)
        gn.series[:] = 7
        sp = pkg.PrachNomaGainSpec(bins, width, lo, ng, reserved)
        hdr = (pkg.PrachNomaGain * max(ng, 1))()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        gp = None if groups is None else (C.c_int32 * len(cfgs))(*groups)
        ser = gn._series()
        if null == "series5":
            ser[5] = None
        args = dict(cfgs=(pkg.PrachCfg * len(cfgs))(*cfgs), res=(pkg.PrachResult * len(cfgs))(), spec=C.byref(sp), hdr=hdr, series=ser)
        if null in args:
            args[null] = None
        rc = L.prach_run_trials_noma_gain(None, args["cfgs"], n, args["res"], None, args["spec"], gp, args["hdr"], args["series"])
        assert (gn.series == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)  # nothing is written by a refusal
        return rc

    good = [noma(), noma(flags=2)]  # (PRACH_FLAG_NOMA_NONSECTOR is accepted)
    assert call(good) == ERR_ARG  # (only the engine is missing)
    for ok in (dict(ngroups=3, groups=[2, 0]), dict(bins=4096, width=1, ngroups=1, groups=[0, 0]), dict(lo=-2 ** 31), dict(lo=2 ** 31 - 1, width=2 ** 31 - 1, bins=4096), dict(bins=1, width=1)):
        assert call(good, **ok) == ERR_ARG, ok  # accepted too
    for kw in (dict(bins=0), dict(bins=-1), dict(bins=4097), dict(width=0), dict(width=-5), dict(ngroups=0), dict(ngroups=-1), dict(ngroups=3), dict(ngroups=1),
               dict(groups=[0, 2], ngroups=2), dict(groups=[-1, 0], ngroups=2), dict(reserved=1), dict(null="cfgs"), dict(null="res"), dict(null="spec"), dict(null="hdr"),
               dict(null="series"), dict(null="series5"), dict(n=0), dict(n=-1)):
        assert call(good, **kw) == ERR_ARG, kw
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        assert call([noma(), pkg.make_cfg(500, variant=variant, rng_mode=pkg.RNG_PHILOX)]) == ERR_UNSUPPORTED
        assert call([pkg.make_cfg(500, variant=variant, rng_mode=pkg.RNG_GLIBC)]) == ERR_UNSUPPORTED
    assert call([noma(), pkg.make_cfg(500, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]) == ERR_UNSUPPORTED
    assert call(good, bins=4096, ngroups=911, groups=[0, 910]) == ERR_UNSUPPORTED  # 36 x 911 x 4096 words > 2^27
    assert call(good, bins=4096, ngroups=910, groups=[0, 909]) == ERR_ARG            # 36 x 910 x 4096 <= 2^27: only the engine is missing
    assert call(good, bins=0, ngroups=911, groups=[0, 910]) == ERR_ARG               # a bad spec comes before UNSUPPORTED
    assert call([noma(), pkg.make_cfg(500, variant=0, rng_mode=pkg.RNG_PHILOX)], bins=0) == ERR_ARG


def test_definition_argument_and_refusal_matrix(pkg, trials):
    L = pkg.lib()
    c, res, a, sched, E, lv = trials[0]
    ptr = a.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
    gn = pkg.NomaGain(1, 50, 300, -16200)
    hdr = pkg.PrachNomaGain()
    lvp = lv.ctypes.data_as(C.c_void_p)

    def logs(sp=None, cfg=c, n=c.nUE, p=ptr, h=hdr, ser=None):
        sp = gn.spec() if sp is None else sp
        return L.prach_noma_gain_accumulate_logs(C.byref(sp) if sp != "null" else None, C.byref(cfg), res.steps, p, n, C.byref(h) if h is not None else None,
                                                 gn._series(0) if ser is None else ser)

    def levels(sp=None, cfg=c, n=c.nUE, p=ptr, h=hdr, ser=None, lp=lvp):
        sp = gn.spec() if sp is None else sp
        return L.prach_noma_gain_accumulate_levels(C.byref(sp) if sp != "null" else None, C.byref(cfg), res.steps, p, n, lp, C.byref(h) if h is not None else None,
                                                   gn._series(0) if ser is None else ser)

    for fn in (logs, levels):
        for bad in (pkg.PrachNomaGainSpec(0, 5, 0, 1, 0), pkg.PrachNomaGainSpec(4097, 5, 0, 1, 0), pkg.PrachNomaGainSpec(50, 0, 0, 1, 0), "null"):
            assert fn(sp=bad) == ERR_ARG
        assert fn(n=c.nUE - 1) == ERR_ARG and fn(p=None) == ERR_ARG and fn(h=None) == ERR_ARG and fn(ser=(C.POINTER(C.c_uint64) * 6)()) == ERR_ARG
        for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
            assert fn(cfg=pkg.make_cfg(c.nUE, variant=variant, rng_mode=pkg.RNG_PHILOX)) == ERR_UNSUPPORTED
    assert levels(lp=None) == ERR_ARG
    glibc = pkg.make_cfg(c.nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)
    assert logs(cfg=glibc) == ERR_UNSUPPORTED  # the gain exists only inside the launch ...
    assert not gn.series.any() and hdr.trials == 0
    assert levels(cfg=glibc) == 0 and hdr.trials == 1  # ... while the levels as given work in any RNG mode
    assert logs() == 0 and hdr.trials == 2 and hdr.ues == 2 * c.nUE and hdr.level_max == int(lv[N.classes(a) != N.IDLE].max())


def test_cli_messages(pkg, tmp_path):
    """--census-gain is refused with the census's messages under --rng glibc, for another --program and next to another reduction, before a device is asked for."""
    out = str(tmp_path / "gain.csv")

    def run(*args):
        p = subprocess.run([pkg.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and not os.path.exists(out)
        return p.stdout

    assert "--census-gain needs --rng philox" in run("--program", "noma", "--rng", "glibc", "--census-gain", out)
    for program in ("beta", "withnoma"):
        assert "--census-gain needs --program noma" in run("--program", program, "--census-gain", out)
    assert "--census-gain needs --program noma" in run("--census-gain", out)
    for other in ("--cdf", "--timeline", "--sojourn", "--ci", "--trace", "--xtab", "--pick", "--census", "--census-ci", "--census-pick", "--census-trace", "--census-timeline"):
        assert "--census-gain cannot be combined with another reduction: one reduction per call" in run("--program", "noma", "--census-gain", out, other, str(tmp_path / "o.csv"))
    for opt, bad in (("--census-gain-bins", "0"), ("--census-gain-bins", "4097"), ("--census-gain-width", "0")):
        assert opt in run("--program", "noma", "--census-gain", out, opt, bad)


def test_kernel_symbols_and_registers(pkg):
    """The two kernels are members of families the library already has, in all three libraries; neither spills nor uses scratch; and the cut sweep's census of
    kernel symbols classes them with the reducers without an edit.  (Fails without the feature: the symbols do not exist.)"""
    import isa_registers as I
    import cut_cases
    if not I.tools_present():
        pytest.skip("llvm-objdump / llvm-readobj / c++filt not found")
    for lib in ("libprach_hip.so", "libprach_hip_tinyq.so", "libprach_hip_nobitop3.so"):
        path = os.path.join(os.path.dirname(pkg.LIB_PATH), lib)
        if not os.path.exists(path):
            import __graft_entry__ as g
            g.build()
        meta = I.metadata(path)
        mine = sorted(k for k in meta if "NomaGain" in k)
        assert mine == ["noma_census_kernel<NomaGainUes, 0>", "noma_census_kernel<NomaGainUes, 1>", "noma_columns_kernel<NomaGainLevels>"], (lib, mine)
        for k in mine:
            assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["private_segment_fixed_size"] == 0 and meta[k]["sgpr_spill_count"] == 0, (lib, k, meta[k])
        assert not cut_cases.check_symbols(set(meta))
    for sym in ("prach_run_trials_noma_gain", "prach_noma_gain_level", "prach_noma_gain_levels", "prach_noma_gain_accumulate_levels", "prach_noma_gain_accumulate_logs",
                "prach_noma_gain_merge", "prach_noma_gain_format_csv", "prach_noma_gain_tile_ues", "prach_noma_gain_lds_max_bins"):
        assert sym in pkg.EXPORTS and hasattr(pkg.lib(), sym)


def test_the_gpu_tests_seeds_stay_clear_of_the_band(pkg):
    """The GPU engine tests require noma_gain_host_ues below 1 % of the arrived UEs.  From the fractional parts of 1000 ln g of the host's table: on the seeds
    those tests use, the UEs within ten bands of an integer (a device-built table moves a product by far less than one band) are far below that share."""
    worst = 0.0
    for n, seeds in ((300, GPU_SEEDS_300), (3000, GPU_SEEDS_3000)):
        for s in seeds:
            c = product_cfg(pkg, n, s, {})
            lg = pkg.noma_activation_table(c)[3]
            assert np.array_equal(pkg.noma_gain_levels(c), G.level_of(lg))
            p = GC.product_of(lg)
            d = p - np.floor(p)
            near = (d <= 10 * GC.BAND) | (d >= 1 - 10 * GC.BAND)
            worst = max(worst, near.sum() / n)
    assert worst < 0.001, worst  # (the expected share is 2 x 10 x 1e-8)


def test_sanitised_stand_alone_run(tmp_path):
    """tests/tools/noma_gain_host_check.c with csrc/prach_host.c under AddressSanitizer and UBSan, as a program of its own on the CPU: exit status 0."""
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = tmp_path / "noma_gain_host_check"
    src = [os.path.join(ROOT, "tests", "tools", "noma_gain_host_check.c"), os.path.join(ROOT, "5g-nr-randomaccess_amd", "csrc", "prach_host.c")]
    # (the sanitizer's runtime is linked into the program itself: nothing has to be loaded in front of it)
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", *src, "-o", str(exe),
                           "-lm", "-lpthread"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "noma_gain_host_check: ok" in p.stdout
