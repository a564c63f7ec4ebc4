"""The two kernels of prach_noma_gain.hip on per-UE state, levels and ln(gain) values no NOMA.c trial leaves behind: tests/tools/gpu_noma_gain_harness.hip
launches them directly on the cases of tests/tools/noma_gain_cases.py — one launch per child process, one child at a time, each under its own timeout.  The
reducer's every output equals the numpy restatement integer for integer under both schemes, the host definition where it applies, and the other scheme.  The
level pre-pass writes the host's level for every UE and lists exactly the UEs inside the band (on both sides of an integer and on it), without a level or
outside the derived range, and none of those just outside the band; with one more EDGE UE than the list holds it reports the count, fills the list and leaves
the words behind it alone.  After an abnormal end no further child is started.  tests/test_noma_gain_cases_cpu.py holds the references without a GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_gain_cases as GC  # noqa: E402
import noma_gain_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return GC.build_harness(tmp_path_factory.mktemp("noma_gain_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in GC.cases(pkg)}


@pytest.fixture(scope="module")
def level_cases():
    return {c.name: c for c in GC.level_cases()}


@pytest.mark.parametrize("name", GC.CASE_NAMES)
def test_reducer_equals_reference_under_both_schemes(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    assert G.identity(ref)
    host = case.host_definition(pkg) if case.host else None
    path = str(tmp_path / "case.bin")
    GC.write_case(case, path)
    outs = []
    for scheme in (0, 1):
        with latch.child(f"{name} scheme {scheme}"):
            out = GC.run_harness(harness, case, path, scheme, tmp_path)
        outs.append(out)
        assert G.same(out, ref) is None, f"scheme {scheme} against numpy: {G.same(out, ref)}"
        if host is not None:
            assert G.same(out, host) is None, f"scheme {scheme} against the host definition: {G.same(out, host)}"
    assert G.same(outs[1], outs[0]) is None


@pytest.mark.parametrize("name", GC.LEVEL_CASE_NAMES)
def test_level_pre_pass_writes_the_hosts_levels_and_lists_the_edge_ues(pkg, harness, level_cases, tmp_path, name):
    case = level_cases[name]
    path = str(tmp_path / "case.bin")
    GC.write_case(case, path)
    with latch.child(f"{name} levels"):
        count, pairs, guard, levels = GC.run_harness(harness, case, path, 2, tmp_path)
    want = case.expected_levels()
    assert np.array_equal(levels, want), np.flatnonzero(levels != want)[:8]
    lg = np.concatenate([j.lgain for j in case.jobs])
    some = np.random.default_rng(7).permutation(len(lg))[:500]
    assert [pkg.noma_gain_level(float(lg[i])) for i in some] == levels[some].tolist()  # ... which are the host function's
    edges = case.expected_edges()
    assert count == len(edges)  # the count goes on past the capacity
    assert (guard == GC.PATTERN).all()  # no write behind the list
    assert len(set(pairs)) == len(pairs) == min(count, case.cap) and set(pairs) <= edges
    if count <= case.cap:
        assert set(pairs) == edges and case.inside <= set(pairs) and not (case.outside & set(pairs))  # inside the band: listed; just outside: nowhere
    else:
        assert count == case.cap + 1  # one more than the list holds
