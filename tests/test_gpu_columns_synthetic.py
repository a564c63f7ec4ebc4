"""prach::columns_kernel on per-UE state no simulation leaves behind: tests/tools/gpu_columns_harness.hip launches the kernel directly on the cases of
tests/tools/columns_cases.py — one launch per child process, one child at a time — and every word of every column, the guard words in front of and behind
every trial's segment included, every offset and every class count equals the numpy restatement integer for integer, and the host definition
(prach_columns_from_logs) where it applies.  tests/test_columns_cases_cpu.py holds the references against the host definition without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import columns_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return CC.build_harness(tmp_path_factory.mktemp("columns_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in CC.cases(pkg)}


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_kernel_equals_reference(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    host = case.host_definition(pkg) if case.host else None
    path = str(tmp_path / "case.bin")
    CC.write_case(case, path)
    with latch.child(name):
        out = CC.run_harness(harness, case, path, tmp_path)
    assert CC.same(out, ref) is None, f"against numpy: {CC.same(out, ref)}"
    if host is not None:
        assert CC.same(out, host) is None, f"against the host definition: {CC.same(out, host)}"
