"""prach::summary_kernel on per-UE state no simulation leaves behind: tests/tools/gpu_summary_harness.hip launches the kernel directly on the cases of
tests/tools/summary_cases.py — both workgroup shapes, one launch per child process, one child at a time — and every row equals the numpy restatement
integer for integer, the host definition (prach_summary_from_logs) where it applies, and the other shape.  tests/test_summary_cases_cpu.py holds the
references against the host definition without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import summary_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return SC.build_harness(tmp_path_factory.mktemp("summary_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in SC.cases(pkg)}


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_kernel_equals_reference_under_both_shapes(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    host = case.host_definition(pkg) if case.host else None
    path = str(tmp_path / "case.bin")
    SC.write_case(case, path)
    outs = []
    for threads in SC.THREADS:
        with latch.child(f"{name} threads {threads}"):
            out = SC.run_harness(harness, case, path, threads, tmp_path)
        outs.append(out)
        assert SC.same(out, ref) is None, f"{threads} threads against numpy: {SC.same(out, ref)}"
        if host is not None:
            assert SC.same(out, host) is None, f"{threads} threads against the host definition: {SC.same(out, host)}"
    assert SC.same(outs[1], outs[0]) is None
