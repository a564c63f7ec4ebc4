"""NOMA.c's channel trace without a GPU: the exact CPU reference (tests/tools/noma_trace_ref.py) checks itself on the first trial cases — the two views of a
trial, the sector hook and the stopped runs, agree on the singletons, and the identities of the record hold on the oracle's UEs; prach_noma_trace_merge and
prach_noma_trace_format_csv against a literal block; the call refuses what it refuses before it needs a device; and prach::noma_kernel's register metadata in
all three libraries is no worse than the build before the recording went in, prach::noma_trace_kernel has neither spill nor scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import noma_trace_ref as R  # noqa: E402

# figures of the cases, from the oracle: (slot, sector) pairs with a singleton, pairs, pairs of which one UE decoded, grants
FIGURES = {"all_states": (1653, 131, 44, 1740), "all_states_partial": (1653, 131, 44, 1740), "cellwide": (837, 129, 48, 918)}


@pytest.mark.parametrize("case", ["all_states", "all_states_partial", "cellwide"])
def test_reference_checks_itself(ob, case):
    oc, res, rows, mask, ues = R.case_trial(ob, case)  # (the self-check of the two views is made inside, at every sampled slot)
    assert mask.sum() >= 50 and len(rows) == R.nslots(res.steps, oc.accessTime)
    R.check_identities(rows, mask, oc.nGrantUL, oc.nPreamble)
    got = (int((rows[..., R.SINGLES] > 0).sum()), int(rows[..., R.PAIRS].sum()), int(rows[..., R.PAIR_ONE].sum()), int(rows[..., R.GRANTED].sum()))
    assert got == FIGURES[case] and got[3] == R.grants_of_ues(ues)
    if case == "cellwide":
        assert not rows[:, 1:].any() and int((rows[mask][..., R.USED] - rows[mask][..., R.SINGLES]).sum()) == 66  # collided bins on the sampled eighth of the slots
    if case == "all_states_partial":
        assert oc.max_steps == 4323 and len(rows) == 865


def test_rebin_of_hand_made_rows():
    rows = np.zeros((4, 6, 6), dtype=np.int64)
    rows[0, 0] = (3, 2, 1, 1, 0, 0)
    rows[1, 5] = (5, 3, 2, 2, 1, 1)
    rows[3, 0] = (7, 3, 2, 1, 1, 0)
    series, sc = R.rebin([rows, rows[:2]], [5, 10], 2, 7, groups=[0, 0], ngroups=2)
    # trial 0: slots at 0, 5, 10, 15 ms -> bins 0, 0, 1, 2 (behind); trial 1: slots at 0, 10 ms -> bins 0, 1
    assert series[R.TX, 0, 0].tolist() == [6, 0] and series[R.TX, 0, 5].tolist() == [5, 5] and int(sc["overflow_tx"][0]) == 7 and int(sc["tx_max"][0]) == 7
    assert [int(sc[f][0]) for f in R.SCALARS] == [2, 6, 23, 13, 8, 7, 3, 2, 7, 7] and int(sc["tx_max"][1]) == -1 and not series[:, 1].any()


def filled(pkg):
    a, b = pkg.NomaTrace(1, 3, 10), pkg.NomaTrace(1, 3, 10)
    a.series[:, 0, 0, 0] = (4, 3, 2, 2, 1, 0)
    a.series[:, 0, 2, 0] = (1, 1, 1, 1, 0, 0)
    a.series[:, 0, 5, 2] = (9, 4, 1, 1, 0, 0)
    for f, v in zip(pkg.NOMA_TRACE_FIELDS, (1, 400, 17, 8, 4, 4, 1, 0, 3, 9)):
        a.scalars[f][0] = v
    b.series[:, 0, 0, 0] = (2, 2, 2, 2, 1, 1)
    b.series[:, 0, 1, 1] = (6, 2, 0, 0, 0, 0)
    for f, v in zip(pkg.NOMA_TRACE_FIELDS, (2, 55, 8, 4, 2, 2, 1, 1, 0, 6)):
        b.scalars[f][0] = v
    return a, b


CSV = b"""p,tx,0,0,6
p,tx,2,0,1
p,tx,all,0,7
p,tx,1,10,6
p,tx,all,10,6
p,tx,5,20,9
p,tx,all,20,9
p,used,0,0,5
p,used,2,0,1
p,used,all,0,6
p,used,1,10,2
p,used,all,10,2
p,used,5,20,4
p,used,all,20,4
p,singles,0,0,4
p,singles,2,0,1
p,singles,all,0,5
p,singles,5,20,1
p,singles,all,20,1
p,granted,0,0,4
p,granted,2,0,1
p,granted,all,0,5
p,granted,5,20,1
p,granted,all,20,1
p,pairs,0,0,2
p,pairs,all,0,2
p,pair_one,0,0,1
p,pair_one,all,0,1
p,tx,all,overflow,3
"""


def test_merge_and_csv_against_a_literal_block(pkg):
    a, b = filled(pkg)
    ab, ba = filled(pkg)[0].merge(b), filled(pkg)[1].merge(a)
    assert ab.same_as(ba)  # exact in any order
    assert [int(ab.scalars[f][0]) for f in pkg.NOMA_TRACE_FIELDS] == [3, 455, 25, 12, 6, 6, 2, 1, 3, 9]
    assert pkg.noma_trace_csv(ab, labels=["p"]) == CSV
    empty = pkg.NomaTrace(1, 3, 10)
    assert pkg.noma_trace_csv(empty) == b"" and int(empty.scalars["tx_max"][0]) == -1
    assert filled(pkg)[0].merge(empty).same_as(a) and empty.merge(a).same_as(a)  # (an empty group's maximum is -1, whatever it holds)
    with pytest.raises(ValueError):
        a.merge(pkg.NomaTrace(1, 4, 10))
    assert np.allclose(ab.collision_ratio(0), [1 / 6, 1.0, 0.75]) and np.isnan(ab.noma_share(0)[1]) and np.allclose(ab.noma_share(0)[[0, 2]], [3 / 5, 0.0])


def test_refusals_need_no_device(pkg):
    """Spec, groups and variants are judged before the engine is looked at: with a NULL engine the refusals of the census come word for word, and an
    acceptable call ends with PRACH_ERR_ARG for the missing engine."""
    L = pkg.lib()
    noma = lambda **kw: pkg.make_cfg(500, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1, **kw)

    def call(cfgs, bins=100, bin_ms=5, ngroups=None, groups=None, reserved=0):
        n = len(cfgs)
        ng = n if ngroups is None else ngroups
        tr = pkg.NomaTrace(max(ng, 1), min(max(bins, 1), 8), bin_ms)
        tr.series[:] = 7
        sp = pkg.PrachNomaTraceSpec(bins, bin_ms, ng, reserved)
        hdr = (pkg.PrachNomaTrace * max(ng, 1))()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        gp = None if groups is None else (C.c_int32 * n)(*groups)
        rc = L.prach_run_trials_noma_trace(None, (pkg.PrachCfg * n)(*cfgs), n, (pkg.PrachResult * n)(), None, C.byref(sp), gp, hdr, tr._series())
        assert (tr.series == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)  # nothing is written by a refusal
        return rc

    good = [noma(), noma()]
    assert call(good) == -1  # (only the engine is missing)
    for kw in (dict(bins=0), dict(bins=pkg.TRACE_MAX_BINS + 1), dict(bin_ms=0), dict(ngroups=0), dict(ngroups=3), dict(groups=[0, 2], ngroups=2), dict(reserved=1)):
        assert call(good, **kw) == -1, kw
    assert call([noma(), pkg.make_cfg(500, variant=0, rng_mode=pkg.RNG_PHILOX)]) == -2
    assert call([noma(), pkg.make_cfg(500, variant=1, rng_mode=pkg.RNG_PHILOX)]) == -2
    assert call([noma(), pkg.make_cfg(500, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]) == -2
    assert call(good, bins=65536, bin_ms=1, ngroups=64, groups=[0, 63]) == -2  # 36 x 64 x 65536 words > 2^27
    assert pkg.noma_trace_tile_rows() % 6 == 0


# prach::noma_kernel as the commit before the recording built it (this toolchain, gfx950), library by library: the recording may cost scalar registers, never a
# vector spill or scratch on the resolver's chain
BEFORE = {"libprach_hip.so": dict(vgpr_spill_count=0, private_segment_fixed_size=0), "libprach_hip_tinyq.so": dict(vgpr_spill_count=0, private_segment_fixed_size=0),
          "libprach_hip_nobitop3.so": dict(vgpr_spill_count=0, private_segment_fixed_size=0)}


@pytest.mark.parametrize("lib", sorted(BEFORE))
def test_register_metadata(pkg, lib):
    import isa_registers as I
    if not I.tools_present():
        pytest.skip("llvm-objdump / llvm-readobj / c++filt not found")
    path = os.path.join(os.path.dirname(pkg.LIB_PATH), lib)
    if lib == "libprach_hip_nobitop3.so" and not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    meta = I.metadata(path)
    for f, v in BEFORE[lib].items():
        assert meta["noma_kernel"][f] <= v, (lib, f, meta["noma_kernel"])
    for k in ("trace_kernel<NomaRows, 0>", "trace_kernel<NomaRows, 1>"):  # (prach::noma_trace_kernel: its symbols are members of the trace_kernel family)
        assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["private_segment_fixed_size"] == 0 and meta[k]["sgpr_spill_count"] == 0, (lib, k, meta[k])
