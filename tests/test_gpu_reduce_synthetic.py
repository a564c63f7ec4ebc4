"""prach::dist_kernel and prach::timeline_kernel on per-UE state no simulation leaves behind: tests/tools/gpu_reduce_harness.hip launches the two kernels
directly on the cases of tests/tools/reduce_cases.py — every binning scheme, one launch per child process — and every output equals the numpy reference
integer for integer, the host definition (prach_dist_accumulate_logs / prach_timeline_accumulate_logs) where it applies, and the other schemes.
tests/test_reduce_cases_cpu.py holds the references against the host definitions without a GPU.  Below that, the two edges a simulation does reach:
preamble counts spread over a whole wavefront and past the last bin, and a truncated trial with whole tiles of UEs that never arrived."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import reduce_cases as R  # noqa: E402
import timeline_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return R.build_harness(tmp_path_factory.mktemp("reduce_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in R.dist_cases() + R.timeline_cases(pkg)}


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", R.DIST_CASE_NAMES + R.TIMELINE_CASE_NAMES)
def test_kernel_equals_reference_under_every_scheme(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    host = case.host_definition(pkg) if case.host else None
    assert case.host or case.kind == "timeline"  # (the definition of the distributions takes every case)
    path = str(tmp_path / "case.bin")
    R.write_case(case, path)
    outs = []
    for scheme in ((0, 1, 2) if case.kind == "dist" else (0, 1)):
        with latch.child(f"{name} scheme {scheme}"):
            out = R.run_harness(harness, case, path, scheme, tmp_path)
        outs.append(out)
        assert case.same(out, ref) is None, f"scheme {scheme} against numpy: {case.same(out, ref)}"
        if host is not None:
            assert case.same(out, host) is None, f"scheme {scheme} against the host definition: {case.same(out, host)}"
    for out in outs[1:]:
        assert case.same(out, outs[0]) is None


# ---- the edges a simulation reaches, through the engine ------------------------------------------------------------------------------------------------

# Beta.c, 2000 UEs, two grants, a 2 ms RAR window, backoff 3, arrivals every millisecond, maxMsg2TxCount = 255, Philox seed 7 (found with the oracle among
# seeds 0..199, LABNOTES): 1584 successful UEs with 197 distinct preamble counts, two of them exactly 255 and two above (the largest 382: every count
# from 255 on shares the last bin)
PTC_CFG = dict(variant=0, maxMsg2TxCount=255, maxRarWindow=2, backoff=3, accessTime=1, nGrantUL=2)
PTC_SEED, PTC_UES = 7, 2000
PTC_EXPECT = dict(success=1584, distinct=197, largest=382, at_255=2, above_255=2, ptc_sum=46338, delay_sum=163657)

_oracle = {}


def ptc_oracle(ob):
    if "ptc" not in _oracle:
        res, ues = ob.run_trial(ob.make_cfg(PTC_UES, **PTC_CFG), ob.Rng(ob.RNG_PHILOX, PTC_SEED))
        _oracle["ptc"] = (res, T.as_array(ues).copy())
    return _oracle["ptc"]


@pytest.mark.parametrize("cluster", [0, 4], ids=["batch", "cluster4"])
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_preamble_counts_spread_and_past_the_last_bin(pkg, ob, eng, scheme, cluster):
    """The batch kernel's 32-byte records (form 1) and the cluster kernels' int32 array (form 0), under every binning scheme: against the logs of the same
    call, numpy on them, and the oracle."""
    eng.set("dist_scheme", scheme)
    if cluster:
        eng.set("cluster", cluster)
    cfg = pkg.make_cfg(PTC_UES, rng_mode=pkg.RNG_PHILOX, seed=PTC_SEED, **PTC_CFG)
    res, logs, d = eng.run_trials_dist([cfg], 4096, 1, want_logs=True)
    tm = eng.timing()
    assert res[0].status == 0 and tm.dist_ms > 0
    assert (tm.rec_mode == 4) == (cluster == 0), (tm.rec_mode, tm.cluster_size, tm.fallback_trials)
    a = T.as_array(logs[0])
    p = a[a[:, R.FLAG] == 1, R.PTC]
    got = dict(success=int(d.success[0]), distinct=len(np.unique(p)), largest=int(p.max()), at_255=int((p == 255).sum()), above_255=int((p > 255).sum()),
               ptc_sum=int(d.ptc_sum[0]), delay_sum=int(d.delay_sum[0]))
    assert got == PTC_EXPECT and got["distinct"] >= 64
    assert int(d.ptc_hist[0, 255]) == PTC_EXPECT["at_255"] + PTC_EXPECT["above_255"]
    assert d.same_as(pkg.dist_from_logs(logs, 4096, 1))
    assert d.same_as(R.bincount_dist(pkg, [a], 4096, 1, [0], 1))
    ores, oues = ptc_oracle(ob)
    assert d.same_as(R.bincount_dist(pkg, [oues], 4096, 1, [0], 1))
    assert (ores.nSuccessUE, ores.preambleTxCount, ores.sumTimer) == (got["success"], got["ptc_sum"], got["delay_sum"])


@pytest.mark.parametrize("rng", [0, 1], ids=["glibc", "philox"])
def test_truncated_trial_leaves_whole_tiles_without_an_arrival(pkg, ob, eng, rng):
    """20 000 UEs stopped after 2500 subframes: the UEs of the second and third tile never arrived.  Both schemes, against the oracle."""
    tile = pkg.timeline_tile_ues()
    c = pkg.make_cfg(20000, variant=1, rng_mode=rng, seed=9, max_steps=2500)
    sched = pkg.arrival_schedule(c)[0]
    ores, oues = ob.run_trial(T.oracle_cfg(ob, c), ob.Rng(rng, 9))
    exp = T.numpy_timeline(pkg, [T.as_array(oues)], [sched], [c.accessTime], 2002, 5)
    tls = []
    for scheme in (0, 1):
        eng.set("timeline_scheme", scheme)
        res, logs, t = eng.run_trials_timeline([c], 2002, 5, want_logs=True)
        a = T.as_array(logs[0])
        assert res[0].status == 0 and eng.timing().timeline_ms > 0
        assert 0 < res[0].activeCheck == ores.activeCheck <= tile and (a[tile:, T.ACTIVE] == -1).all() and (a[:ores.activeCheck, T.ACTIVE] != -1).all()
        assert t.same_as(pkg.timeline_from_logs([c], logs, 2002, 5)), (T.describe(t), scheme)
        assert t.same_as(T.numpy_timeline(pkg, [a], [sched], [c.accessTime], 2002, 5))
        assert t.same_as(exp), (T.describe(t), T.describe(exp))
        assert int(t.scalars["arrived"][0]) == ores.activeCheck and int(t.scalars["success"][0]) == ores.nSuccessUE > 0
        tls.append(t)
    assert tls[1].same_as(tls[0])
