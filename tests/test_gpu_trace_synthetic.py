"""prach::trace_kernel on rows no trial writes: tests/tools/gpu_trace_harness.hip launches the kernel directly on its own cases — every lane of a tile near
2^31 - 1 so that the 64-bit sums are exercised, rows one subframe shorter and longer than a tile, a bin wider than the row, all-zero rows, subframes behind
the last bin, jobs without subframes between the others — under both binning schemes, one launch per child process, one child at a time; every output
word equals the harness's plain host loop."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = ["huge_values_full_tile", "huge_values_one_bin", "tile_minus_one", "tile_plus_one", "tile_edges_bin7", "bin_wider_than_row", "all_zero",
         "overflow_behind_bins", "jobs_without_subframes"]
_abnormal = []  # a harness run that ended abnormally (a HIP error, a signal, a timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path_factory.mktemp("trace_harness") / "gpu_trace_harness")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tests", "tools", "gpu_trace_harness.hip"), "-o", exe])
    return exe


def test_case_list_and_tile(harness, pkg):
    assert subprocess.check_output([harness, "--cases"], text=True).split() == CASES
    consts = dict(l.split() for l in subprocess.check_output([harness, "--constants"], text=True).splitlines())
    assert int(consts["TR_TILE"]) == pkg.trace_tile_subframes()


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_host_loop_under_both_schemes(harness, name):
    for scheme in (0, 1):
        assert not _abnormal, f"not started: {_abnormal[0]}"
        try:
            p = subprocess.run([harness, name, str(scheme)], capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired as e:
            _abnormal.append(f"{name} scheme {scheme}: {e}")
            raise
        if p.returncode not in (0, 1):
            _abnormal.append(f"{name} scheme {scheme}: exit {p.returncode}: {p.stderr[-1000:]}")
        assert p.returncode == 0 and p.stdout.strip().endswith(": ok"), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
