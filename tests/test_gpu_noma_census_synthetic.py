"""prach::noma_census_kernel and prach::noma_columns_kernel on per-UE state no NOMA.c trial leaves behind: tests/tools/gpu_noma_census_harness.hip launches
the kernels directly on the cases of tests/tools/noma_census_cases.py — the census under both schemes and the columns, one launch per child process, one
child at a time, each under its own timeout — and every output equals the numpy restatement integer for integer, the host definitions where they apply, and
the other scheme.  After an abnormal end no further child is started.  tests/test_noma_census_cases_cpu.py holds the references against the host definitions
without a GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_census_cases as NC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return NC.build_harness(tmp_path_factory.mktemp("noma_census_harness"))


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in NC.cases(pkg)}


def launch(harness, case, path, mode, out_dir, name):
    with latch.child(f"{name} {mode}"):
        return NC.run_harness(harness, case, path, mode, out_dir)


@pytest.mark.parametrize("name", NC.CASE_NAMES)
def test_kernels_equal_reference_under_both_schemes(pkg, harness, cases, tmp_path, name):
    case = cases[name]
    ref = case.reference()
    host = case.host_definition(pkg) if case.host else None
    path = str(tmp_path / "case.bin")
    NC.write_case(case, path)
    outs = []
    for scheme in (0, 1):
        out = launch(harness, case, path, scheme, tmp_path, name)
        outs.append(out)
        assert NC.same(out, ref) is None, f"scheme {scheme} against numpy: {NC.same(out, ref)}"
        if host is not None:
            assert NC.same(out, host) is None, f"scheme {scheme} against the host definition: {NC.same(out, host)}"
    assert NC.same(outs[1], outs[0]) is None
    data, counts = launch(harness, case, path, "columns", tmp_path, name)
    rd, rc = case.reference_columns()
    assert np.array_equal(data, rd) and np.array_equal(counts, rc), "columns against numpy"
    if case.host:
        hd, hc = case.host_columns(pkg)
        assert np.array_equal(data, hd) and np.array_equal(counts, hc), "columns against the host definition"
