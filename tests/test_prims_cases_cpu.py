"""tests/tools/prims_cases.py and tests/tools/gpu_prims_harness.hip without a GPU: both harness builds compile for gfx950 and carry the constants the
generator assumes; the Philox reference reproduces the Random123 vectors; over the WHOLE record enumeration of the mask section the `light` predicate
written from the comment above pass_masks agrees with what the branched per-UE body (the harness's --host mode) does to a record, and light, no-op and heavy
records are each at least 1 % of it; the sector boundaries exist and the statement is monotone; the grids of the `blocks` section
are the launchers'; the host paths of fastmod / slot_align / pack / unpack equal their references.  tests/test_gpu_prims_synthetic.py runs the same cases
on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import prims_cases as P  # noqa: E402


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return P.build_harness(tmp_path_factory.mktemp("prims_harness"))  # both builds compile for gfx950


@pytest.fixture(scope="module")
def consts(harness):
    return P.harness_constants(harness["product"])


def _host(harness, section, n, payload, tmp_path, **kw):
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "res.bin")
    P.write_case(case, section, n, payload, **kw)
    P.run_harness(harness["product"], section, case, res, host=True)
    return P.read_result(res, section, 1, n).astype(np.int64)


def test_both_builds_carry_the_constants_the_generator_assumes(harness, consts):
    assert P.harness_constants(harness["nobitop3"]) == consts
    c = consts
    assert (c["PK_ACT_SHIFT"], c["PK_CONN_SHIFT"], c["PK_PRE_SHIFT"], c["PK_RAR_SHIFT"], c["PK_MRC_SHIFT"], c["PK_PEND_SHIFT"]) == (0, 2, 4, 12, 20, 28)
    assert c["PK_GRANT_BIT"] == 1 << 31 and c["PK_PEND_SHIFT"] + 3 == 31  # the grant bit sits right above the 3-bit deferred outcome
    assert sorted(c[k] for k in ("ACT_IDLE", "ACT_DONE", "ACT_M1", "ACT_M3")) == [0, 1, 2, 3]
    assert [c[k] for k in ("PEND_NONE", "PEND_STAY", "PEND_CALLER", "PEND_RESET", "PEND_PASSIVE", "PEND_RJOIN")] == [0, 1, 2, 3, 4, 5]  # "pend 0..2" of the predicate
    assert c["UEV_NONE"] == 0 and c["GR_NONE"] == 0xFFFFF and c["HOT_BO_BIAS"] > 0 and c["SPIN_LIMIT"] > 0
    assert c["CLUSTER_LQCAP"] % 64 == 0 and c["CLUSTER_MAX_G"] == 64 and c["PRIMS_THREADS"] % 64 == 0
    assert P.MASK_MAXMSG2 + 1 <= 0xff and max(P.MASK_MAXRAR) + 1 + 3 <= 0xff  # every enumerated field fits its byte, aged


def test_philox_reference_reproduces_the_known_answers(ob):
    cases = P.philox_cases()
    assert 15000 <= len(cases) <= 20000 and len(np.unique(cases, axis=0)) > len(cases) - 10
    for ctr, key, exp in P.PHILOX_KAT:
        assert P.philox_block(ob, ctr, key) == exp
    ref = P.philox_reference(ob, cases[:3])
    assert ref[:, 0].tolist() == [exp[0] >> 1 for _, _, exp in P.PHILOX_KAT]
    # what a trial never feeds: full-width words everywhere, seed_hi != 0, c1 at the wrap
    assert (cases[:, 1] != 0).sum() > 10000 and (cases[:, 3] == 0xFFFFFFFF).sum() >= 41 and (cases[:, 3] == 0xFFFFFFFE).sum() >= 41
    assert (cases[:, 2] == 2**24 - 1).sum() >= 12 and set(cases[-100:, 5].tolist()) <= {0, 1, 2, 3}


@pytest.fixture(scope="module")
def whole_enumeration(harness, consts, tmp_path_factory):
    M = P.mask_cases(consts, full=True)
    d = tmp_path_factory.mktemp("masks_host")
    case, res = str(d / "case.bin"), str(d / "res.bin")
    P.write_masks(case, M)
    P.run_harness(harness["product"], "masks", case, res, host=True, timeout=600)
    return M, P.MaskTable(M, P.read_result(res, "masks", 1, M.n), consts)


def test_enumeration_covers_what_it_claims(whole_enumeration, consts):
    M, T = whole_enumeration
    plain = np.arange(M.n) < 64 * M.nplain
    assert (M.recs[plain, 0] == 0).all() and 3_900_000 < plain.sum() < 4_500_000
    for t in P.MASK_T:
        for maxRar in P.MASK_MAXRAR:
            k = plain & (T.t == t) & (T.maxRar == maxRar)
            f = P.enum_decode(M.recs[k, 1], t, maxRar, consts)
            # the numpy restatement of the decoder is the harness's (what --host echoes is what it ran on)
            assert (f["pk"] == T.pk[k]).all() and (f["rx"] == T.rx[k]).all() and (f["rz"] == T.rz[k]).all() and f["valid"].all()
            assert len(np.unique(M.recs[k, 1])) == P.enum_decode(  # (every valid record; a few twice, to fill the last wavefront)
                np.arange(P.enum_size(maxRar)), t, maxRar, consts)["valid"].sum()
            vals = {k: set(np.unique(f[k]).tolist()) for k in ("act", "conn", "pre", "pend", "rar", "mrc", "grant", "rx", "rz")}
            assert vals["act"] == {0, 1, 2, 3} and vals["conn"] == {0, 1, 2} and vals["pre"] == set(P.MASK_PRE) and vals["pend"] == set(range(6))
            assert vals["rar"] == set(range(maxRar + 2)) and vals["mrc"] == {0, P.MASK_MAXMSG2, P.MASK_MAXMSG2 + 1} and vals["grant"] == {0, 1}
            assert vals["rx"] == set(range(t - 4, t + 3)) and vals["rz"] == {-2, 0, 1, t - 1, t, t + 1, t + 5}
            stay = f["pend"] == consts["PEND_STAY"]
            assert (f["rx"][stay] <= t - 1).all() and set(np.unique(f["rx"][stay]).tolist()) == set(range(t - 4, t))


def test_light_predicate_and_body_agree_over_the_whole_enumeration(whole_enumeration, consts):
    """predicate => the body leaves exactly the light path's state; and where the deferred outcome does not consult the caller tables (pend 0..2, no
    grant), the body leaving that state => predicate.  (A PEND_PASSIVE / PEND_RJOIN record that the tables happen to bump ends in the same state: that is the
    tables' doing, phase B's business, and the predicate rightly says no.)"""
    M, T = whole_enumeration
    plain = np.arange(M.n) < 64 * M.nplain
    bad = plain & T.pred & ~T.light_state
    assert not bad.any(), f"{bad.sum()} light records the body treats otherwise, first {np.flatnonzero(bad)[:5]}"
    own = plain & (T.f["pend"] <= 2) & (T.f["grant"] == 0)
    bad = own & T.light_state & ~T.pred
    assert not bad.any(), f"{bad.sum()} records in the light state the predicate misses, first {np.flatnonzero(bad)[:5]}"
    assert not (T.pred & T.noop).any()  # (a light record changes: rar + 1)
    assert not (T.pred_spec & ~T.pred).any() and (T.pred & ~T.pred_spec & plain).sum() > 10000
    n = plain.sum()
    light, quiet = (T.pred & plain).sum(), (T.noop & plain).sum()
    heavy = n - light - quiet
    assert min(light, quiet, heavy) >= 0.01 * n, (light, quiet, heavy, n)
    # the window-closing records and the aged ones are there (what the `<` and the age term of pass_masks decide)
    age = np.where(T.f["pend"] == consts["PEND_STAY"], T.t - 1 - T.rx, 0)
    contending = plain & (T.f["pend"] <= 2) & (T.f["grant"] == 0) & (T.f["act"] == consts["ACT_M1"]) & (T.f["pre"] != 0) & (T.rz <= T.t)
    assert (contending & (T.f["rar"] + age + 1 == T.maxRar)).sum() > 1000 and (contending & (T.f["rar"] + age + 2 == T.maxRar) & (age > 0)).sum() > 1000


def test_the_sample_of_the_gpu_test_is_the_enumerations(consts):
    M = P.mask_cases(consts)
    assert 1_000_000 <= 64 * M.nplain <= 2_000_000 and M.n % 64 == 0
    fronts = M.groups[M.groups[:, 2] == 1]
    lanes = {(int(g[5] - g[3]), int(g[4] - g[3]), int(g[6] - g[3])) for g in fronts}
    assert lanes == {(a, b, c) for a in P.FRONT_LANES for b in P.FRONT_LANES for c in P.FRONT_LANES if a <= b <= c}
    for g in np.flatnonzero(M.twin >= 0):
        assert (M.recs[64 * g:64 * g + 64] == M.recs[64 * M.twin[g]:64 * M.twin[g] + 64]).all() and M.groups[M.twin[g], 2] == 0
    k = np.random.default_rng(0).integers(0, M.nplain, 200)
    mixed = [len(set(P.fields_of(P.enum_decode(M.recs[64 * g:64 * g + 64, 1], M.groups[g, 0], M.groups[g, 1], consts)["pk"], consts)["pend"])) for g in k]
    assert min(mixed) >= 4  # a wavefront mixes classes


def test_sector_boundaries_exist_and_the_statement_is_monotone():
    b = P.sector_boundaries()
    assert b == sorted(b) and len(set(b)) == 5 and 0 < b[0] and b[-1] < P.INT_MAX
    for k, d in enumerate(b, start=1):
        assert P.sector_reference(d - 1) == k - 1 and P.sector_reference(d) == k
    d = np.sort(P.sector_cases())
    s = P.sector_reference(d)
    assert (np.diff(s) >= 0).all() and set(s) == set(range(6)) and s[0] == 0 and s[-1] == 5
    grid = np.arange(0, 2**31, 4099, dtype=np.int64)
    assert (np.diff(P.sector_reference(grid)) >= 0).all()
    # about a sixth each, but for the reference's 3.14: sector 5 ends at 2 * 3.14f
    assert [int(v) for v in np.round(np.diff([0] + b + [2**31]) / 2**31 * 6)] == [1] * 6


def test_block_grids_are_the_launchers(consts):
    exprs = P.launcher_grid_expressions()
    for G, xpack, ntrials, grid in P.block_sets().tolist():
        for name, expr in exprs.items():
            assert P.eval_c_grid(expr, G, xpack, ntrials) == grid == P.launch_grid(G, xpack, ntrials), (name, G, xpack, ntrials)
        assert grid >= G * ntrials and grid <= 1 << 17
    assert len(P.block_sets()) == 84


def test_mod_host_paths_equal_python(harness, tmp_path):
    cases = P.mod_cases()
    assert set(P.MOD_DIVISORS) <= set(cases[:, 1].tolist()) and set(cases[:, 3].tolist()) == set(range(1, 21))
    assert (cases[:, 2] >= 0).all() and (cases[:, 0] == 2**32 - 1).sum() >= len(P.MOD_DIVISORS)
    r = _host(harness, "mod", len(cases), [cases], tmp_path).reshape(-1, 8)
    mod, sa = P.mod_reference(cases)
    assert (r[:, 0] == mod).all() and (r[:, 1] == mod).all()
    assert (r[:, 2] == sa).all() and (r[:, 3] == sa).all() and (r[:, 4] == sa).all()
    d = cases[:, 1]
    assert (r[:, 5] == np.where(d > 1, 2**32 // d, 0xFFFFFFFF)).all()  # make_fastmod


def test_pack_unpack_host_path_equals_bit_slicing(harness, consts, tmp_path):
    cases = P.pack_cases()
    r = _host(harness, "pack", len(cases), [cases], tmp_path).reshape(-1, 13)
    f = P.fields_of(cases[:, 3], consts)
    for k in range(3):
        assert (r[:, k] == cases[:, k]).all() and (r[:, 10 + k] == cases[:, k]).all()
    for k, name in enumerate(("act", "conn", "pre", "rar", "mrc", "pend"), start=3):
        assert (r[:, k] == f[name]).all(), name
    assert (r[:, 9] == (cases[:, 3] & 0x7FFFFFFF)).all()  # pack(unpack(r)) drops the grant bit, which is not a field of the state, and nothing else


def test_small_generators_hold_what_they_are_there_for(consts):
    names = [n for n, _ in P.wave_cases()]
    assert len(set(names)) == len(names) and sum(n.startswith("one_hot_") for n in names) == 64 and sum(n.startswith("random_") for n in names) >= 200
    g = P.granule_cases(consts)
    made = g[g[:, 0] == 0]
    assert set(made[:, 3].tolist()) >= set(range(0x10000)) and ((made[:, 3] & 0xFFFF) != (made[:, 4] & 0xFFFF)).all()
    pairs = {(int(a), int(b)) for a, b in made[:5 * 0x10000, 1:3]}
    assert len(pairs) == 25
    w0, w1, ok, probe = P.granule_reference(g)
    assert ok[g[:, 0] == 0].all() and not probe[g[:, 0] == 0].any() and not ok[g[:, 0] == 1].any()
    h = P.hot_cases(consts)
    assert (h[:, 3] == 0).sum() == 20 and (h[h[:, 3] == 1, 2] >> 31).any()
    assert len(P.slot_pairs(consts)) == 64 * 65 // 2
