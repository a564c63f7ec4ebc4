"""The device code that decides who gets a grant on inputs no trial produces: tests/tools/gpu_resolve_harness.hip runs prach::noma_resolve_sector (mode 1),
the restatement inside prach::noma_glibc_slot (mode 2) and prach::classify_event + prach::resolve_reset_candidates<1 | 4> (mode 3) on the named cases of
tests/tools/resolve_cases.py — every case of a mode in ONE launch, one launch per child process, six child processes in all.  Granted set, draws taken and
status equal the pinned oracle's per-sector function exactly, the two NOMA copies equal each other, and every output word of the reset-candidate resolver
equals the sequential definition.  tests/test_resolve_cases_cpu.py holds the cases and the references themselves without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import resolve_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return R.build_harness(tmp_path_factory.mktemp("resolve_harness"))


@pytest.fixture(scope="module")
def consts(harness):
    return R.harness_constants(harness)


def _child(harness, case_path, result_path, devact, what):
    with latch.child(what):
        R.run_harness(harness, case_path, result_path, devact, timeout=120)


@pytest.fixture(scope="module")
def noma(ob, consts):
    cases = R.noma_cases(consts)
    refs = {c.name: R.case_reference(ob, c, consts) for c in cases}
    units = [(c, s, refs[c.name][0][s].budget) for c in cases for s in sorted(c.sectors) if refs[c.name][0][s].reached]
    return cases, refs, units


@pytest.fixture(scope="module")
def shared_runs(harness, consts, noma, tmp_path_factory):
    """Mode 1 under devact 0, 1, 2: {devact: {(case name, sector): result}}.  A launch that fails raises here: every test that needs this fixture errors, and no
    later child is started."""
    cases, refs, units = noma
    d = tmp_path_factory.mktemp("mode1")
    path = str(d / "cases.bin")
    R.write_mode1(path, units, consts)
    out = {}
    for devact in (0, 1, 2):
        res = str(d / f"result{devact}.bin")
        _child(harness, path, res, devact, f"mode 1 devact {devact}")
        out[devact] = {(c.name, s): r for (c, s, _), r in zip(units, R.read_mode1(res, units, consts, devact))}
    return out


@pytest.fixture(scope="module")
def glibc_runs(harness, noma, tmp_path_factory):
    """Mode 2 under devact 0, 1: {devact: {case name: result}}."""
    cases, refs, _ = noma
    d = tmp_path_factory.mktemp("mode2")
    path = str(d / "cases.bin")
    R.write_mode2(path, cases, [refs[c.name][1] for c in cases])
    out = {}
    for devact in (0, 1):
        res = str(d / f"result{devact}.bin")
        _child(harness, path, res, devact, f"mode 2 devact {devact}")
        out[devact] = {c.name: r for c, r in zip(cases, R.read_mode2(res, cases, devact))}
    return out


def _check_noma(case, ref, shared, glibc, consts):
    """None, or what differs: both copies against the reference (and so each other), devact = 0."""
    secs, _, used, status = ref
    bad = []
    for s in sorted(case.sectors):
        r = secs[s]
        if r.reached:
            g = shared[(case.name, s)]
            if (g["granted"], g["taken"], g["status"]) != (r.grants, r.taken, r.status):
                bad.append(f"shared copy, sector {s}: granted {g['granted']} taken {g['taken']} status {g['status']}; reference {r.grants} {r.taken} {r.status}")
            if g["ambiguous"]:
                bad.append(f"shared copy, sector {s}: ambiguous with a host-built table")
        want = r.grants if r.reached else []
        if glibc["granted"][s] != want:
            bad.append(f"glibc copy, sector {s}: granted {glibc['granted'][s]}; reference {want}" + ("" if r.reached else " (behind the exhausted sector)"))
        if r.reached and glibc["granted"][s] != (shared[(case.name, s)]["granted"] if shared[(case.name, s)]["status"] == consts["PRACH_OK"] else []):
            bad.append(f"sector {s}: the two copies differ")
    if (glibc["pos"], glibc["status"]) != (used, status):
        bad.append(f"glibc copy: position {glibc['pos']} status {glibc['status']}; reference {used} {status}")
    return "; ".join(bad) or None


@pytest.mark.parametrize("name", R.NOMA_CRAFTED_NAMES)
def test_noma_copies_equal_the_reference(noma, shared_runs, glibc_runs, consts, name):
    cases, refs, _ = noma
    case = next(c for c in cases if c.name == name)
    assert _check_noma(case, refs[name], shared_runs[0], glibc_runs[0][name], consts) is None


def test_noma_copies_equal_the_reference_random_sweep(noma, shared_runs, glibc_runs, consts):
    cases, refs, _ = noma
    bad = {c.name: m for c in cases if c.name.startswith("random_") for m in [_check_noma(c, refs[c.name], shared_runs[0], glibc_runs[0][c.name], consts)] if m}
    assert not bad, f"{len(bad)} cases: " + " | ".join(f"{k}: {v}" for k, v in list(bad.items())[:4])


def test_stream_exhaustion(noma, shared_runs, glibc_runs, consts):
    """PRACH_ERR_STREAM, no grant of the exhausted sector, the earlier sectors' grants stand; a budget of exactly the draws needed succeeds."""
    cases, refs, _ = noma
    ERR, OK = consts["PRACH_ERR_STREAM"], consts["PRACH_OK"]
    seen = 0
    for c in cases:
        secs, _, used, status = refs[c.name]
        g2 = glibc_runs[0][c.name]
        if status != ERR:
            assert g2["status"] == OK, c.name
            continue
        seen += 1
        last = max(s for s in secs if secs[s].reached)
        assert g2["status"] == ERR and shared_runs[0][(c.name, last)]["status"] == ERR, c.name
        assert g2["granted"][last] == [] == shared_runs[0][(c.name, last)]["granted"] and g2["pos"] == used, c.name
        for s in secs:
            assert g2["granted"][s] == (secs[s].granted if s < last else []), (c.name, s)
    assert seen >= 8
    assert glibc_runs[0]["budget_exactly_enough"]["status"] == OK and shared_runs[0][("budget_exactly_enough", 3)]["status"] == OK
    later = refs["six_sectors_budget_ends_in_a_later_sector"][0]
    assert sum(len(r.granted) for r in later.values() if r.reached and r.status == OK) > 0  # earlier sectors did grant


def test_device_built_table_reports_the_bands(noma, shared_runs, glibc_runs, consts):
    """devact = 1: grants unchanged, `ambiguous` exactly where two sorted neighbours lie within ACT_GAIN_ORDER_BAND or a difference lies within 1e-9 of
    15 — by name on the crafted cases and their twins just outside, by the definition (resolve_cases.sector_reference) on every case."""
    cases, refs, _ = noma
    OK, AMB = consts["PRACH_OK"], consts["NOMA_GLIBC_AMBIGUOUS"]
    flagged = {}
    for c in cases:
        secs, _, used, status = refs[c.name]
        want_status, want_pos, live = OK, 0, True
        for s in sorted(secs):
            r = secs[s]
            if r.reached:
                g = shared_runs[1][(c.name, s)]
                assert (g["granted"], g["taken"], g["status"]) == (r.grants, r.taken, r.status), (c.name, s)
                if r.status == OK:
                    assert g["ambiguous"] == int(r.ambiguous), (c.name, s, g["ambiguous"])
                    flagged.setdefault(c.name, []).append(g["ambiguous"])
            if live:  # the glibc copy stops behind the first sector that is exhausted or ambiguous; that sector's grants are applied unless exhausted
                assert glibc_runs[1][c.name]["granted"][s] == r.grants, (c.name, s)
                want_pos += len(r.taken)
                if r.status != OK:
                    want_status, live = r.status, False
                elif r.ambiguous:
                    want_status, live = AMB, False
            else:
                assert glibc_runs[1][c.name]["granted"][s] == [], (c.name, s)
        assert (glibc_runs[1][c.name]["status"], glibc_runs[1][c.name]["pos"]) == (want_status, want_pos), c.name
    for name in R.AMBIGUOUS_NAMES:
        assert flagged[name] == [1] and glibc_runs[1][name]["status"] == AMB, name
    for name in R.CLEAR_TWIN_NAMES:
        assert flagged[name] == [0] and glibc_runs[1][name]["status"] == OK, name


def test_ambiguity_hook_flags_every_sort(noma, shared_runs, consts):
    """devact = 2: every sector that sorts at least two singletons is ambiguous; grants unchanged."""
    cases, refs, _ = noma
    n = 0
    for c in cases:
        for s, r in refs[c.name][0].items():
            if r.reached:
                g = shared_runs[2][(c.name, s)]
                assert (g["granted"], g["taken"], g["status"]) == (r.grants, r.taken, r.status), (c.name, s)
                if r.status == consts["PRACH_OK"]:
                    assert g["ambiguous"] == int(r.count > c.nG and r.count >= 2), (c.name, s)
                    n += g["ambiguous"]
    assert n > 1000


@pytest.fixture(scope="module")
def reset(harness, consts, tmp_path_factory):
    cases = R.reset_cases(consts)
    d = tmp_path_factory.mktemp("mode3")
    path, res = str(d / "cases.bin"), str(d / "result.bin")
    R.write_mode3(path, cases)
    _child(harness, path, res, 0, "mode 3")
    return {c.name: (c, r) for c, r in zip(cases, R.read_mode3(res, cases))}


@pytest.mark.parametrize("name", R.RESET_CASE_NAMES)
def test_reset_candidates_equal_the_sequential_definition(reset, consts, name):
    case, got = reset[name]
    ref = R.reset_reference(case, consts)
    if case.only_count:  # more survivors than RCCAP: the kernels end the trial there; only the count is defined
        assert (got["nrc"], got["resolved"]) == (ref["nrc"], 0) and ref["nrc"] > consts["RCCAP"]
        return
    for key in ("nrc", "nrj", "resolved", "nlv", "fie", "fcall", "void"):
        if got[key] != ref[key]:
            where = [k for k, (a, b) in enumerate(zip(got[key], ref[key])) if a != b][:8] if isinstance(ref[key], list) else ""
            pytest.fail(f"{name} (NB = {case.NB}, nP = {case.nP}): {key} differs from the sequential definition {where}")
