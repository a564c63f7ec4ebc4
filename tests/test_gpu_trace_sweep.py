"""The per-subframe preamble trace through the drivers: prach_sim --trace (one worker and two forked workers merged through the shared mapping) and
sweep.py --trace (one rank and two ranks rehearsed on one GPU under gloo) write the CSV of the oracle's reference (tests/tools/trace_ref.py), byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import trace_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

POINTS, TIMES, BIN = [1000, 2000], 2, 5


@pytest.fixture(scope="module")
def expected(pkg):
    """Beta.c, Philox, the drivers' grid: one group per sweep point over the seeds; txop = calls and collisions = calls - singles at every subframe."""
    bins = 10000 // BIN
    t = pkg.Trace(len(POINTS), bins, BIN)
    for k, n in enumerate(POINTS):
        for s in range(TIMES):
            r = TR.ref((0, n, {}, 1, s), 1)
            wx, wq = r.weighted()
            for name, per in (("calls", r.calls), ("singles", r.singles), ("txop", wx), ("collisions", wq)):
                b, over = TR.binned(per, bins, BIN)
                assert over == 0
                t.series[name][k] += b.astype(np.uint64)
    return t.csv(labels=POINTS)


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_trace(pkg, expected, tmp_path, workers):
    out = tmp_path / "trace.csv"
    p = subprocess.run([pkg.CLI_PATH, "--program", "beta", "--rng", "philox", "--times", str(TIMES), "--sweep", "1000:2000:1000", "--out", str(tmp_path), "--logs", "0",
                        "--trace", str(out)] + (["--devices", "0,0"] if workers == 2 else []), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-2000:])
    assert out.read_bytes() == expected and len(expected) > 1000


@pytest.mark.parametrize("world", [1, 2])
def test_sweep_driver_trace(pkg, expected, tmp_path, world):
    out = tmp_path / "trace.csv"
    sweep = [os.path.join(ROOT, "5g-nr-randomaccess_amd", "sweep.py"), "--times", str(TIMES), "--sweep", "1000:2000:1000", "--out", str(tmp_path), "--backend", "gloo",
             "--same-device", "--trace", str(out)]
    launcher = [sys.executable] if world == 1 else [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                                    "--master-port", "29547"]
    p = subprocess.run(launcher + sweep, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert out.read_bytes() == expected
    if world == 1:
        bad = subprocess.run([sys.executable] + sweep + ["--ci", str(out)], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and "--trace cannot be combined" in bad.stderr
