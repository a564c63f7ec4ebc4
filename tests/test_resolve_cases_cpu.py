"""tests/tools/resolve_cases.py without a GPU: the case names are fixed and the generator is deterministic; every crafted case holds what it is for, read off
the reference's own output; the random sweep reaches pairs, leftovers and more pairs than grants in the shares asserted below; the oracle's per-sector
entry (oracle/noma_oracle.c: noma_oracle_group_sector) is the function a whole NOMA oracle trial runs, shown by replaying that trial's sectors; and
tests/tools/gpu_resolve_harness.hip compiles for gfx950 and carries the constants the generator used."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import resolve_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def consts(tmp_path_factory):
    """hipcc --offload-arch=gfx950 on the harness, which pulls in prach_noma_glibc.hip, prach_noma_resolve.h and prach_resolve.h as they are; nothing is launched."""
    return R.harness_constants(R.build_harness(tmp_path_factory.mktemp("resolve_harness")))


@pytest.fixture(scope="module")
def noma(ob, consts):
    cases = R.noma_cases(consts)
    return {c.name: c for c in cases}, {c.name: R.case_reference(ob, c, consts) for c in cases}


@pytest.fixture(scope="module")
def reset(consts):
    cases = R.reset_cases(consts)
    return {c.name: c for c in cases}, {c.name: R.reset_reference(c, consts) for c in cases}


def test_harness_compiles_and_carries_the_generators_constants(consts):
    assert 0 < consts["ACT_GAIN_ORDER_BAND"] < 1e-12  # (the order-band cases are placed at 0.75 and 1.5 times the compiled value)
    assert consts["RCCAP"] == 256 == max(R.SURVIVOR_COUNTS) and consts["M1_WORDS"] == 452 and consts["M1_RES"] == 196 and consts["NUE_BYTES"] == 80
    assert len({consts[k] for k in ("UEV_NONE", "UEV_CALLER", "UEV_RESETCAND", "UEV_RJOIN", "EV_LEAVER")}) == 5
    assert all(0 <= consts[k] < 8 for k in ("UEV_NONE", "UEV_CALLER", "UEV_RESETCAND", "UEV_RJOIN", "EV_LEAVER"))
    assert consts["PRACH_OK"] == 0 and consts["PRACH_ERR_STREAM"] < 0 and consts["NOMA_GLIBC_AMBIGUOUS"] not in (0, consts["PRACH_ERR_STREAM"])


def test_case_names_are_fixed_and_the_generator_is_deterministic(consts, noma, reset):
    assert tuple(noma[0]) == R.NOMA_CASE_NAMES and tuple(reset[0]) == R.RESET_CASE_NAMES
    assert len(set(R.NOMA_CASE_NAMES)) == len(R.NOMA_CASE_NAMES) and len(set(R.RESET_CASE_NAMES)) == len(R.RESET_CASE_NAMES)
    for a, b in zip(R.noma_cases(consts), noma[0].values()):
        assert (a.nP, a.nG, a.nonsector, a.budget, a.rows, a.pos0) == (b.nP, b.nG, b.nonsector, b.budget, b.rows, b.pos0) and sorted(a.sectors) == sorted(b.sectors)
        for s in a.sectors:
            x, y = a.sectors[s], b.sectors[s]
            assert np.array_equal(x.pre, y.pre) and np.array_equal(x.gain, y.gain) and np.array_equal(x.draws, y.draws) and x.collided == y.collided
            assert np.array_equal(a.uid[s], b.uid[s])
    for a, b in zip(R.reset_cases(consts), reset[0].values()):
        assert (a.nP, a.NB) == (b.nP, b.NB) and np.array_equal(a.fcall, b.fcall) and np.array_equal(a.events, b.events)


def _only(refs, name):
    secs = refs[name][0]
    assert len(secs) == 1
    return next(iter(secs.values()))


def test_reference_and_plain_python_walk_agree(noma):
    """The oracle's sort and pairing against python_walk (a direct reading of NOMA.c:251-307) on every sector: the same UEs end up paired and left over."""
    cases, refs = noma
    n = 0
    for name, c in cases.items():
        for s, r in refs[name][0].items():
            if r.count <= c.nG:
                assert r.granted == list(range(r.count)) and not r.consumed
                continue
            sec = c.sectors[s]
            order, l10, pairs, looked, left = R.python_walk(sec.gain, r.logs, c.nG)
            want = set()
            for g, (i, j) in enumerate(pairs[:c.nG]):
                d1, d2 = int(sec.draws[g, 0]), int(sec.draws[g, 1])
                want |= {order[i], order[j]} if d1 > R.D1_LOW else ({order[i]} if c.nonsector else {order[(i, j)[d2 % 2]]})
            want |= {order[k] for k in left[:max(0, c.nG - len(pairs))]}
            assert set(r.granted) == want, (name, s)
            assert r.consumed == [(g, w) for g in range(min(len(pairs), c.nG)) for w in ((0, 1) if sec.draws[g, 0] <= R.D1_LOW and not c.nonsector else (0,))], (name, s)
            n += 1
    assert n > 2000


def test_crafted_noma_cases_hold_what_they_are_for(noma, consts):
    cases, refs = noma
    nG0 = cases["count_1"].nG
    assert [_only(refs, f"count_{k}").count for k in ("1", "2", "ngrant", "ngrant_plus_1", "63", "64")] == [1, 2, nG0, nG0 + 1, 63, 64]
    assert cases["count_63"].nP == cases["count_64"].nP == 64 and _only(refs, "count_ngrant").consumed == [] and _only(refs, "count_ngrant").granted == [0, 1, 2]
    r = _only(refs, "count_64_pairs_lane_63")
    assert r.count == 64 and r.pair_list == [(0, 63)] and len(r.granted) == 41 and {r.order[0], r.order[63]} <= set(r.granted)
    r = _only(refs, "tie_all_equal")
    assert r.pairs == 0 and r.granted == [0, 1] and r.ambiguous  # stable: the first two in preamble order
    r = _only(refs, "tie_decides_who_pairs")  # the low UE pairs the FIRST of the two equal gains in preamble order; the other gets nothing
    assert r.order == [1, 0, 2] and r.pair_list == [(0, 1)] and r.granted == [0, 1] and r.ambiguous
    r = _only(refs, "chain_nearest_admissible")
    assert r.pair_list == [(0, 2), (1, 3), (4, 6), (5, 7)] and r.consumed == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)] and len(r.granted) == 5
    r = _only(refs, "nobody_pairs")
    assert r.pairs == 0 and r.leftovers_granted == 3 and r.granted == sorted(r.order[:3]) and not r.consumed
    r, c = _only(refs, "lane0_only_admissible_partner"), cases["lane0_only_admissible_partner"]
    sec = c.sectors[0]
    assert r.pairs == 0 and R.python_walk(sec.gain, sec.lg, c.nG, jstart=0)[2] == [(1, 0)]  # (what a partner search that starts at lane 0 would pair)
    for name in ("more_pairs_than_grants", "more_pairs_than_grants_nonsector"):
        r = _only(refs, name)
        assert r.pairs == 3 > cases[name].nG == 1 and r.leftovers_granted == 0 and len(r.granted) == 1 and (r.count - 2 * r.pairs) == (name.endswith("nonsector"))
    r = _only(refs, "collided_preambles_stay_out")
    assert r.count == 4 and len(cases["collided_preambles_stay_out"].rows) == 4 + 2 * 3
    for q, g_lo in enumerate(R.G_LOS):
        a, b = (cases[f"threshold_{q}_{k}"].sectors[q % 6 if q != 3 else 0].gain[0] for k in ("below", "above"))
        assert np.nextafter(a, np.inf) == b and not R.pairs_with(g_lo, a) and R.pairs_with(g_lo, b)
        for label, pairs, amb in (("below", 0, True), ("above", 1, True), ("minus_1e-10", 0, True), ("plus_1e-10", 1, True), ("minus_1e-8", 0, False), ("plus_1e-8", 1, False)):
            r = _only(refs, f"threshold_{q}_{label}")
            assert (r.pairs, r.ambiguous) == (pairs, amb) and len(r.granted) == 1 + pairs and len(r.consumed) == pairs, (q, label)
            d = abs(10 * r.logs[0] - 10 * r.logs[1] - 15.0)
            assert d < 1e-13 if label in ("below", "above") else 0.5e-10 < d < 2e-10 if "1e-10" in label else 0.5e-8 < d < 2e-8
    for q in range(3):
        assert _only(refs, f"order_band_{q}_inside").ambiguous and not _only(refs, f"order_band_{q}_outside").ambiguous
        g = np.sort(cases[f"order_band_{q}_inside"].sectors[q].gain)
        assert 0 < g[1] - g[0] <= consts["ACT_GAIN_ORDER_BAND"] * g[1]
    assert {n for n in R.NOMA_CRAFTED_NAMES if any(r.ambiguous for r in refs[n][0].values())} == set(R.AMBIGUOUS_NAMES)
    assert not set(R.CLEAR_TWIN_NAMES) & set(R.AMBIGUOUS_NAMES) and set(R.CLEAR_TWIN_NAMES) <= set(R.NOMA_CRAFTED_NAMES)
    # draws: d1 on either side of 0.3, d2 odd and even, both values of nonsector
    for d1 in (0, R.D1_LOW, R.D1_HIGH, R.D_MAX):
        assert (d1 / 2147483647 < 0.3) == (d1 <= R.D1_LOW)
        for par in ("even", "odd"):
            r, rn = _only(refs, f"draws_d1_{d1}_d2_{par}"), _only(refs, f"draws_d1_{d1}_d2_{par}_nonsector")
            assert r.pairs == rn.pairs == 2
            assert r.consumed == ([(0, 0), (0, 1), (1, 0), (1, 1)] if d1 <= R.D1_LOW else [(0, 0), (1, 0)]) and rn.consumed == [(0, 0), (1, 0)]
            assert len(r.granted) == len(rn.granted) == (2 if d1 <= R.D1_LOW else 4)
            if d1 <= R.D1_LOW:
                assert rn.granted == sorted(r.order[i] for i, _ in r.pair_list) and r.granted == sorted(r.order[p[par == "odd"]] for p in r.pair_list)
    # budgets
    OK, ERR = consts["PRACH_OK"], consts["PRACH_ERR_STREAM"]
    for k, label in enumerate(("first_draw_of_grant_0", "second_draw_of_grant_0", "first_draw_of_grant_1", "second_draw_of_grant_1")):
        secs, stream, used, status = refs[f"budget_{label}"]
        r = secs[3]
        assert status == ERR == r.status and used == k and r.taken == [(0, 0), (0, 1), (1, 0), (1, 1)][:k] and r.grants == [] and len(r.granted) == 2
    secs, stream, used, status = refs["budget_exactly_enough"]
    assert status == OK and used == 4 == len(stream) and secs[3].grants == secs[3].granted
    secs, stream, used, status = refs["six_sectors_position_carries"]
    assert status == OK and sum(bool(r.consumed) for r in secs.values()) == 6 and used == len(stream) > 9
    secs, stream, used, status = refs["six_sectors_budget_ends_in_a_later_sector"]
    assert status == ERR and used == 15 and [r.reached for r in secs.values()] == [True] * 3 + [False] * 3 and secs[0].grants and secs[1].grants
    first_bad = min(s for s, r in secs.items() if r.status == ERR)
    assert first_bad == 2 and len(secs[2].taken) == 3 and len(secs[2].consumed) == 6  # in the middle of a sector
    secs, stream, used, status = refs["six_sectors_budget_ends_at_a_sector_start"]
    first_bad = min(s for s, r in secs.items() if r.status == ERR)
    assert status == ERR and used == 6 and secs[first_bad].taken == [] and secs[first_bad].budget == 0 and first_bad == 2


def test_random_sweep_reaches_what_no_trial_does(noma):
    cases, refs = noma
    rs = [(c, r) for n, c in cases.items() if n.startswith("random_") for r in refs[n][0].values() if r.count > c.nG]
    assert len(rs) >= 2000 and len([n for n in cases if n.startswith("random_")]) == R.N_RANDOM
    assert sum(r.pairs >= 1 for _, r in rs) >= len(rs) / 2
    assert sum(r.leftovers_granted >= 1 for _, r in rs) >= len(rs) / 4
    assert sum(r.pairs > c.nG for c, r in rs) >= len(rs) / 10
    counts = {r.count for n in cases if n.startswith("random_") for r in refs[n][0].values()}
    assert counts == set(range(1, 65)) and {c.nG for c in cases.values()} >= set(range(1, 41)) and {c.nonsector for c in cases.values()} == {0, 1}
    assert sum(refs[n][3] != 0 for n in cases if n.startswith("random_")) >= 20  # budgets that run out somewhere


def test_sector_entry_is_what_a_whole_trial_runs(ob):
    """Every sector of whole NOMA oracle trials (both stream forms, the cell-wide variant), replayed through noma_oracle_group_sector with the draws the
    trial took: the same UEs are granted, in the same order, after the same draws."""
    n = paired = 0
    for mode, seed, kw in ((ob.RNG_GLIBC, 3, dict()), (ob.RNG_PHILOX, 11, dict(nGrantUL=3)), (ob.RNG_GLIBC, 5, dict(nonsector=1, nGrantUL=6))):
        cfg = ob.make_noma_cfg(8000, max_steps=2500, **kw)
        res, plain = ob.noma_run_trial(cfg, ob.Rng(mode, seed), want_ues=False)
        res2, sectors = ob.noma_run_trial_traced(cfg, ob.Rng(mode, seed))
        assert res.as_dict() == res2.as_dict() and len(sectors) > 300  # (recording changes nothing)
        for rec in sectors:
            table = np.zeros((cfg.nGrantUL, 2), dtype=np.int32)
            for g, w, v in rec["draws"]:
                table[g, w] = v
            granted, consumed, logs = ob.noma_group_sector(rec["idx"], rec["gain"], cfg.nGrantUL, cfg.nonsector, table)
            assert granted == rec["granted"] and consumed == [(g, w) for g, w, _ in rec["draws"]], (rec["slot"], rec["sector"])
            assert logs.tolist() == [R.clog(g) for g in rec["gain"]]
            n += 1
            paired += bool(consumed)
    assert n > 1500 and paired > 100


def test_reset_cases_hold_what_they_are_for(reset, consts):
    cases, refs = reset
    RC, CALL, LEAVE = consts["UEV_RESETCAND"], consts["UEV_CALLER"], consts["EV_LEAVER"]
    for n in R.SURVIVOR_COUNTS:
        for NB in (1, 4):
            ref = refs[f"survivors_{n}_nb{NB}"]
            assert ref["nrc"] == n and ref["resolved"] == 1 and ref["killed_by_definite"] == 20 and ref["nrj"] == 5
    assert refs["survivors_257_only_counted"]["nrc"] == 257 and refs["survivors_257_only_counted"]["resolved"] == 0 and cases["survivors_257_only_counted"].only_count
    assert refs["survivors_exactly_rccap_few_buckets"]["nrc"] == consts["RCCAP"]
    for NB in (1, 4):
        for label, lead in (("first_rejoins", 0), ("first_bumped", 1)):
            c, ref = cases[f"chain_{label}_nb{NB}"], refs[f"chain_{label}_nb{NB}"]
            ev = c.events[np.argsort(c.events[:, 0])]
            fate = [ref["void"][int(np.flatnonzero(c.events[:, 0] == i)[0])] for i in ev[:, 0]]
            assert all(((ev[k, 1] >> 4) & 0xff) == ((ev[k + 1, 1] >> 12) & 0xff) for k in range(lead, len(ev) - 1))  # p_k = q_(k+1)
            assert fate[0] == 0 and fate[64] == lead and fate[128] == lead if NB == 4 else fate[0] == 0  # the first candidate of the later blocks
            if NB == 4:
                assert fate[lead:] == [k % 2 for k in range(200)] and not np.array_equal(ev[:, 0], c.events[:, 0])  # every fate hangs on the one before; listed shuffled
    c, ref = cases["few_buckets_p_equals_q_nb1"], refs["few_buckets_p_equals_q_nb1"]
    assert any((i & 7) == RC and ((i >> 4) & 0xff) == ((i >> 12) & 0xff) for i in c.events[:, 1].tolist())
    ref = refs["bumped_by_definite_caller_and_by_rejoin"]
    assert ref["killed_by_definite"] >= 30 and ref["bumped_by_rejoin"] >= 30 and ref["nrc"] - ref["bumped_by_rejoin"] >= 10
    c, ref = cases["leavers_and_callers_around_the_first_caller"], refs["leavers_and_callers_around_the_first_caller"]
    lv = [(int(i), (int(w) >> 4) & 0xff) for i, w in c.events.tolist() if (w & 7) == LEAVE]
    assert sum(i == c.fcall[p] - 1 for i, p in lv) >= 20 and sum(i == c.fcall[p] + 1 for i, p in lv) >= 20 and sum(ref["nlv"]) == sum(i < c.fcall[p] for i, p in lv) >= 20
    cl = [(int(i), (int(w) >> 4) & 0xff) for i, w in c.events.tolist() if (w & 7) == CALL]
    assert sum(i == c.fcall[p] for i, p in cl) == sum(ref["fie"]) >= 10 and sum(i > c.fcall[p] for i, p in cl) >= 10
    assert (np.diff(cases["events_in_ascending_order"].events[:90, 0]) > 0).all()
    assert [cases[f"nb1_np{nP}"].nP for nP in R.NB1_NP] == [1, 2, 54, 63, 64]
    for nP in R.NB4_NP:
        c = cases[f"nb4_np{nP}_register_edges"]
        cand = [((int(w) >> 4) & 0xff, (int(w) >> 12) & 0xff) for w in c.events[:, 1].tolist() if (w & 7) == RC]
        regs = set(range((nP + 63) // 64))
        assert {p >> 6 for p, _ in cand} == regs == {q >> 6 for _, q in cand}  # new and old buckets in every register in use
        edges = {b for b in (63, 64, 127, 128, 191, 192) if b < nP} | {nP - 1}
        assert edges <= {p for p, _ in cand} and edges <= {q for _, q in cand}
        assert nP % 64 != 0 or nP == 128 or nP == 192
    rnd = [refs[n] for n in cases if n.startswith("random_")]
    assert len(rnd) == R.N_RESET_RANDOM and sum(r["nrc"] > 64 for r in rnd) >= 40 and sum(bool(r["bumped_by_rejoin"]) for r in rnd) >= 60
