"""prach::noma_summary_kernel and prach::noma_pick_kernel on per-UE state no NOMA.c trial leaves behind: tests/tools/gpu_noma_select_harness.hip launches the
kernels directly on the cases of tests/tools/noma_select_cases.py — each case under both THREADS instantiations, one launch per child process, one child at
a time, each under its own timeout — and every output equals the numpy restatement integer for integer, the host definitions where a case's schedules are
the product's, and the other instantiation.  After an abnormal end no further child is started.  tests/test_noma_select_cases_cpu.py holds the references
against the host definitions without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_select_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return SC.build_harness(tmp_path_factory.mktemp("noma_select_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in SC.cases(pkg)}


def launch(harness, case, path, threads, out_dir):
    with latch.child(f"{case.name} {threads}"):
        return SC.run_harness(harness, case, path, threads, out_dir)


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_kernels_equal_reference_under_both_instantiations(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    host = SC.host_rows(case, case.host_definition(pkg)) if case.host else None
    path = str(tmp_path / "case.bin")
    SC.write_case(case, path)
    outs = []
    for threads in SC.THREADS:
        out = launch(harness, case, path, threads, tmp_path)
        outs.append(out)
        assert SC.same(case, out, ref) is None, f"{threads} threads against numpy: {SC.same(case, out, ref)}"
        if host is not None:
            assert SC.same(case, out, host) is None, f"{threads} threads against the host definition: {SC.same(case, out, host)}"
        if case.kind == "summary":  # what the engine never reads is as the header says: nothing counted for an unused field, -1 in an unused level
            nf, nq = len(case.spec[0]), len(case.spec[2])
            assert all(not any(r["unused"]) and (r["raw_levels"][nf:] == -1).all() and (r["raw_levels"][:, nq:] == -1).all() for r in out)
    assert SC.same(case, outs[1], outs[0]) is None
