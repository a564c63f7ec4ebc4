"""The quiet-subframe path of prach::lcluster_kernel on the GPU: the two base trials of tests/tools/quiet_cases.py, both variants, both RNG modes
(lcluster_kernel<false> and <true>), clusters of 4 and of 16 workgroups, each uncut and stopped at 64 consecutive subframes from the first one with an
off-slot singleton and at 64 more from the first subframe that takes the path; every trial equals the oracle (tests/test_gpu_parity.py's assert_same) and stays on the lean kernel (rec_mode 3, no fallback
trial, no rerun on trial_kernel).  One case per test, each in a fresh child process (tests/tools/gpu_lcluster_quiet.py) under `timeout -k 10`; after
a child that was killed, timed out or died on a signal the remaining cases fail without starting anything.  tests/test_lcluster_quiet_cases_cpu.py
shows without a GPU what the trials contain."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import quiet_cases as QC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a child that ended abnormally (signal, timeout): no later case of this file starts another one

LIMIT = 120  # seconds per case: 129 short oracle runs, the package import and at most 17 calls of small trials take a few seconds together


@pytest.mark.parametrize("cluster", [4, 16])
@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", [b[0] for b in QC.BASES])
def test_quiet_path_equals_oracle(pkg, name, variant, rng, cluster):
    env = dict(os.environ)
    env.pop("PRACH_LIB", None)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "tools", "gpu_lcluster_quiet.py"), name, str(variant), str(rng), str(cluster)]
    p = latch.python_child(f"{name} {variant} {rng} {cluster}", cmd, LIMIT, env)
    assert p.returncode == 0 and p.stdout.splitlines()[-1].startswith(f"done {2 * QC.CUTS + 1} cases 0 bad"), (p.returncode, p.stdout[-4000:], p.stderr[-2000:])
