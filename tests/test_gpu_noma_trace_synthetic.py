"""prach::noma_trace_kernel on (slot, sector) rows no trial writes: tests/tools/gpu_noma_trace_harness.hip launches the kernel directly on the cases of
tests/tools/noma_trace_cases.py — both binning schemes, one launch per child process — and every output equals the numpy reference integer for integer, and the
other scheme; the guard words behind every output keep their pattern.  tests/test_noma_trace_cases_cpu.py holds the reference against the plain loop without a
GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_trace_cases as N  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return N.build_harness(tmp_path_factory.mktemp("noma_trace_harness"))


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in N.cases()}


@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_kernel_equals_reference_under_both_schemes(harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    path = str(tmp_path / "case.bin")
    N.write_case(case, path)
    outs = []
    for scheme in (0, 1):
        with latch.child(f"{name} scheme {scheme}"):
            out = N.run_harness(harness, case, path, scheme, tmp_path)  # (header and guard words: read_result)
        outs.append(out)
        assert N.same(out, ref) is None, f"scheme {scheme} against numpy: {N.same(out, ref)}"
    assert N.same(outs[1], outs[0]) is None
