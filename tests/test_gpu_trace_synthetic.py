"""prach::trace_kernel on rows no trial writes: tests/tools/gpu_trace_harness.hip launches the kernel directly on its own cases — every lane of a tile near
2^31 - 1 so that the 64-bit sums are exercised, rows one subframe shorter and longer than a tile, a bin wider than the row, all-zero rows, subframes behind
the last bin, jobs without subframes between the others — under both binning schemes, one launch per child process, one child at a time; every output
word equals the harness's plain host loop."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ["huge_values_full_tile", "huge_values_one_bin", "tile_minus_one", "tile_plus_one", "tile_edges_bin7", "bin_wider_than_row", "all_zero",
         "overflow_behind_bins", "jobs_without_subframes"]
latch = H.Latch()  # a harness run that ended abnormally (a HIP error, a signal, a timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return H.build("gpu_trace_harness.hip", tmp_path_factory.mktemp("trace_harness"))


def test_case_list_and_tile(harness, pkg):
    assert H.run(harness, ["--cases"]).stdout.split() == CASES
    assert H.constants(harness)["TR_TILE"] == pkg.trace_tile_subframes()


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_host_loop_under_both_schemes(harness, name):
    for scheme in (0, 1):
        with latch.child(f"{name} scheme {scheme}"):
            p = H.run(harness, [name, scheme], ok=(0, 1))  # (1: the outputs differ — the child ended on its own)
        assert p.returncode == 0 and p.stdout.strip().endswith(": ok"), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
