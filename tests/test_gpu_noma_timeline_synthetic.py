"""prach::noma_timeline_kernel on per-UE state no NOMA.c trial leaves behind: tests/tools/gpu_noma_timeline_harness.hip launches the kernel directly on the
cases of tests/tools/noma_timeline_cases.py under both schemes — one launch per child process, one child at a time, each under its own timeout — and every
output equals the numpy restatement integer for integer, the host definition where it applies, and the other scheme.  After an abnormal end no further child
is started.  tests/test_noma_timeline_cases_cpu.py holds the references against the host definition without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_timeline_cases as TC  # noqa: E402
import noma_timeline_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return TC.build_harness(tmp_path_factory.mktemp("noma_timeline_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in TC.cases(pkg)}


@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_kernel_equals_reference_under_both_schemes(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    assert T.identity(ref)
    host = case.host_definition(pkg) if case.host else None
    path = str(tmp_path / "case.bin")
    TC.write_case(case, path)
    outs = []
    for scheme in (0, 1):
        with latch.child(f"{name} scheme {scheme}"):
            out = TC.run_harness(harness, case, path, scheme, tmp_path)
        outs.append(out)
        assert TC.same(out, ref) is None, f"scheme {scheme} against numpy: {TC.same(out, ref)}"
        if host is not None:
            assert TC.same(out, host) is None, f"scheme {scheme} against the host definition: {TC.same(out, host)}"
    assert TC.same(outs[1], outs[0]) is None
