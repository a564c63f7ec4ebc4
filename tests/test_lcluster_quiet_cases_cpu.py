"""The quiet-subframe path of prach::lcluster_kernel, its cases without a GPU (tests/tools/quiet_cases.py): from the oracle's census (Philox, seed 700,
both variants) each base trial holds at least 100 subframes of every kind the branch tells apart — calls and no singleton (the path is taken), a
singleton call off the access subframe (quiet by its events, must fall through), no call at all — and off the access subframe the calls never exceed
nPreamble (they are the buckets' lowest matched members calling again: one wavefront, lane = bucket, sees all of them).  Conditions on the CASES, not
measurements of the library; tests/test_gpu_lcluster_quiet.py runs the same trials on the GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import quiet_cases as QC  # noqa: E402

# (taken, offsingle, nocall) as counted when the cases were chosen: the census is deterministic, so these are exact
EXPECTED = {
    ("at7_g3_2500", 0): (5214, 752, 3579), ("at7_g3_2500", 1): (5233, 625, 3719),
    ("g3_p8_3000", 0): (5547, 812, 1130), ("g3_p8_3000", 1): (5826, 712, 1107),
}


@pytest.fixture(scope="module")
def census(ob):
    return {(name, v): QC.classes(QC.trial(name, v, ob.RNG_PHILOX)) for name, _, _ in QC.BASES for v in (0, 1)}


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", [b[0] for b in QC.BASES])
def test_base_holds_every_kind_of_subframe(census, name, variant):
    c = census[(name, variant)]
    got = tuple(int(c[k].sum()) for k in ("taken", "offsingle", "nocall"))
    print(name, variant, "taken / off-slot singleton / no call:", got)
    assert min(got) >= 100, got
    assert got == EXPECTED[(name, variant)], got


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", [b[0] for b in QC.BASES])
def test_off_slot_calls_never_exceed_the_preambles(census, name, variant):
    c = census[(name, variant)]
    assert int(c["calls"][c["off"]].max()) <= c["nPreamble"]


def test_cuts_start_at_an_off_slot_singleton(ob):
    for name, _, _ in QC.BASES:
        for v in (0, 1):
            for rng in (ob.RNG_GLIBC, ob.RNG_PHILOX):
                case = QC.trial(name, v, rng)
                c, cuts = QC.classes(case), QC.cuts_of(case)
                assert len(cuts) == QC.CUTS and cuts == list(range(cuts[0], cuts[0] + QC.CUTS))
                last = [x - 1 for x in cuts]
                assert c["offsingle"][last[0]] and not c["offsingle"][:last[0]].any()
                # the second window starts where the path is first taken and holds subframes that take it and subframes that fall through
                tk = [x - 1 for x in QC.taken_cuts_of(case)]
                assert c["taken"][tk[0]] and not c["taken"][:tk[0]].any() and len(tk) == QC.CUTS
                assert c["taken"][tk].sum() >= 4 and (c["singles"][tk] > 0).sum() >= 8 and c["nocall"][tk].sum() >= 8, (name, v, rng)
                assert len(QC.all_cuts_of(case)) == 2 * QC.CUTS  # (the windows do not overlap in these trials)
