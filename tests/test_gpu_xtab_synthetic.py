"""prach::xtab_kernel on per-UE state no simulation leaves behind: tests/tools/gpu_xtab_harness.hip launches the kernel directly on the cases of
tests/tools/xtab_cases.py — both schemes, one launch per child process, one child at a time — and every output equals the numpy reference integer for
integer, the host definition (prach_xtab_accumulate_logs) where it applies, and the other scheme.  tests/test_xtab_cases_cpu.py holds the references
against the host definition without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import xtab_cases as XC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return XC.build_harness(tmp_path_factory.mktemp("xtab_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in XC.cases(pkg)}


@pytest.mark.parametrize("name", XC.CASE_NAMES)
def test_kernel_equals_reference_under_both_schemes(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    host = case.host_definition(pkg) if case.host else None
    path = str(tmp_path / "case.bin")
    XC.write_case(case, path)
    outs = []
    for scheme in (0, 1):
        with latch.child(f"{name} scheme {scheme}"):
            out = XC.run_harness(harness, case, path, scheme, tmp_path)
        outs.append(out)
        assert XC.same(out, ref) is None, f"scheme {scheme} against numpy: {XC.same(out, ref)}"
        if host is not None:
            assert XC.same(out, host) is None, f"scheme {scheme} against the host definition: {XC.same(out, host)}"
    assert XC.same(outs[1], outs[0]) is None
