"""The cut sweep on the GPU: every simulation kernel, held on its kernel by engine options (prach_timing checked after every call), runs the base trials of
tests/tools/cut_cases.py stopped at consecutive subframes — max_steps = 1 .. 4 max(accessTime, 5), 64 consecutive cuts in a busy stretch of the trial,
and the cuts around its end — and every stopped trial equals an oracle run cut at the same subframe: every counter, totalDelay, draws, steps, time_exit
and all 16 logged fields of every UE, bit-exact.  One row per test, each in a fresh child process (tests/tools/gpu_cut_sweep.py) under `timeout -k 10`;
after a child that was killed, timed out or died on a signal the remaining rows fail without starting anything.  tests/test_cut_cases_cpu.py shows
without a GPU what the cuts contain; tests/tools/CUT_SWEEP.md has the table of rows and the measured figures."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import cut_cases as CC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a child that ended abnormally (signal, timeout): no later row of this file starts another one

# seconds per row: the oracle's prefix runs (a few seconds on 16 threads), the package import and the GPU calls (measured: tests/tools/CUT_SWEEP.md) take
# well under a minute together; the slot-by-slot NOMA.c form makes one launch per access slot of every trial
LIMIT = 240


@pytest.mark.parametrize("row", [r["name"] for r in CC.CUT_ROWS])
def test_row_equals_oracle_at_every_cut(pkg, row):
    env = dict(os.environ)
    env.pop("PRACH_LIB", None)
    p = latch.python_child(row, [sys.executable, os.path.join(ROOT, "tests", "tools", "gpu_cut_sweep.py"), row], LIMIT, env)
    assert p.returncode == 0 and " 0 bad" in p.stdout.splitlines()[-1], (p.returncode, p.stdout[-6000:], p.stderr[-2000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("row ")]
    assert len(lines) == len(CC.ROW[row].get("pipeline", (None,))) and all(" bad=0 " in l for l in lines), p.stdout[-3000:]
