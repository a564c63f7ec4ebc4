"""The grant sweep on the GPU: every Beta.c / WithNOMA simulation kernel, held on its kernel by engine options with the cluster size the bases need
(prach_timing checked after every call: the pin choose_kernel predicts, no fallback trial, no rerun on trial_kernel), runs the base trials of
tests/tools/grant_cases.py cut at t + 1 and t + 2 behind every chosen subframe t — subframes with 64, 65 and more singleton callers in which the bin form
of the grant selection meets a crossing bin, a bin that ends exactly at the budget, one grant, more grants than callers, the last bin, several sectors
with a crossing bin each — and every stopped trial equals an oracle run cut at the same subframe: every counter, totalDelay, draws, steps, time_exit and
all 16 logged fields of every UE, bit-exact.  One row per test, each in a fresh child process (tests/tools/gpu_cut_sweep.py --grant) under
`timeout -k 10`; after a child that was killed, timed out or died on a signal the remaining rows fail without starting anything.  A trial that leaves its
row's kernel fails its row: none does.  tests/test_grant_cases_cpu.py shows without a GPU what the chosen subframes contain;
tests/tools/GRANT_SWEEP.md has the classes, the coverage table and the measured figures."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import grant_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a child that ended abnormally (signal, timeout): no later row of this file starts another one

# seconds per row.  Measured on the MI355X (GRANT_SWEEP.md): a child takes 1.5-1.9 s in all — the package import, the oracle's 72-84 prefix runs (under 1 s on
# 16 threads: the 240 runs of all rows together take 2.1 s) and the GPU calls (0.2-0.65 s); the cut sweep allows its rows 240 s for up to 5.7 s, the same
# factor of forty-two here
LIMIT = 80


@pytest.mark.parametrize("row", [r["name"] for r in GC.GRANT_ROWS])
def test_row_equals_oracle_behind_every_chosen_subframe(pkg, row):
    env = dict(os.environ)
    env.pop("PRACH_LIB", None)
    p = latch.python_child(row, [sys.executable, os.path.join(ROOT, "tests", "tools", "gpu_cut_sweep.py"), "--grant", row], LIMIT, env)
    assert p.returncode == 0 and " 0 bad" in p.stdout.splitlines()[-1], (p.returncode, p.stdout[-6000:], p.stderr[-2000:])
    r = GC.GROW[row]
    trials = GC.trials_of(r)
    sizes = {s["pin"]["cluster_size"] for s, *_ in trials}
    lines = [l for l in p.stdout.splitlines() if l.startswith("row ")]
    assert len(lines) == len(sizes) * len(r.get("pipeline", (None,))) and all(" bad=0 " in l for l in lines), p.stdout[-3000:]
    # every trial of the row ran, on the row's kernel: the chosen subframes of tests/test_grant_cases_cpu.py's COVERAGE all count
    assert sum(int(re.search(r"cases= *(\d+)", l).group(1)) for l in lines) == len(trials) * len(r.get("pipeline", (None,))), p.stdout[-3000:]
