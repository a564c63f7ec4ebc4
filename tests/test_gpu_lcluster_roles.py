"""The exchange roles of prach::lcluster_kernel on the GPU: the cases of tests/tools/roles_cases.py — cluster sizes and preamble counts at which a
thread's second and third bucket role, the tail loop behind them and the second event role are live, one at which that role is skipped (the headline's
shape), one bucket role only and every row of the bucket tables — each with both variants in both RNG modes (lcluster_kernel<false> and <true>), uncut and
stopped at a handful of subframes; every trial equals the oracle (tests/test_gpu_parity.py's assert_same) and stays on the lean kernel on a cluster of
the case's size (rec_mode 3, no fallback trial, no rerun on trial_kernel).  One case per test, each in a fresh child process
(tests/tools/gpu_lcluster_roles.py) under `timeout -k 10`; after a child that was killed, timed out or died on a signal the remaining cases fail without
starting anything.  tests/test_lcluster_roles_cases_cpu.py shows without a GPU what the trials contain."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import roles_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a child that ended abnormally (signal, timeout): no later case of this file starts another one

LIMIT = 120  # seconds per case: 24 oracle runs of a few thousand UEs, the package import and at most 12 calls of small trials take a few seconds together


@pytest.mark.parametrize("name", [c[0] for c in RC.CASES])
def test_roles_equal_oracle(pkg, name):
    env = dict(os.environ)
    env.pop("PRACH_LIB", None)
    p = latch.python_child(name, [sys.executable, os.path.join(ROOT, "tests", "tools", "gpu_lcluster_roles.py"), name], LIMIT, env)
    print(p.stdout[-1500:])
    assert p.returncode == 0 and p.stdout.splitlines()[-1].startswith(f"done {4 * (1 + len(RC.CUTS))} trials 0 bad"), (p.returncode, p.stdout[-4000:], p.stderr[-2000:])
