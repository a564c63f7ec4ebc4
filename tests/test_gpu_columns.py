"""prach_run_trials_columns on the GPU: the columns prach::columns_kernel writes on the device equal, integer for integer, prach_columns_from_logs of the
per-UE logs the same call returns, the numpy restatement over those logs and over the oracle's UEs: in both RNG modes, behind every simulation kernel, with
trials around the tile in one call, under the reruns the engine knows (a trial is written once), with and without host logs, and — in a child process
that imports torch first — straight into a torch tensor."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import columns_cases as CC  # noqa: E402
import timeline_ref as T  # noqa: E402
from test_gpu_pick import KERNELS as PICK_KERNELS, oracle_trial, trial_cfgs  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = {k: v for k, v in PICK_KERNELS.items() if "pick_threads" not in v}  # the simulation kernels
MENU = ["one", "arrival", "sojourn", "completion", "timer", "ptc", "failcount", "age", "state"]
RAW = ["raw:" + n for n in ("idx", "timer", "active", "txTime", "firstTxTime", "secondTxTime", "nowBackoff", "preamble", "preambleChange", "rarWindow", "maxRarCounter",
                            "preambleTxCounter", "msg2Flag", "connectionRequest", "msg4Flag", "failCount")]
REPEATED = ["sojourn", "raw:timer", "sojourn", "timer", "raw:timer"]
SPECS = [MENU, RAW, REPEATED]
CHILD = os.path.join(ROOT, "tests", "tools", "gpu_columns_device_child.py")


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def numpy_of(pkg, cfgs, arrays, ends, col):
    return np.concatenate([CC.numpy_columns(a, pkg.arrival_schedule(c)[0], c.accessTime, E, col.field_ids) for c, a, E in zip(cfgs, arrays, ends)], axis=1)


def same(a, b):
    return a.fields == b.fields and np.array_equal(a.data, b.data) and all(np.array_equal(a.headers[f], b.headers[f]) for f in a.headers.dtype.names)


def run_checked(pkg, eng, cfgs, fields):
    """One call with logs: the device's columns and headers equal columns_from_logs and numpy on the logs of the same call."""
    res, logs, col = eng.run_trials_columns(cfgs, fields, want_logs=True)
    assert all(r.status == 0 for r in res)
    host = pkg.columns_from_logs(cfgs, [r.steps for r in res], logs, fields)
    arrays = [T.as_array(l) for l in logs]
    assert same(col, host) and np.array_equal(col.data, numpy_of(pkg, cfgs, arrays, [min(r.steps, r.maxTime) for r in res], col))
    assert col.headers["nUE"].tolist() == [c.nUE for c in cfgs] and not col.headers["status"].any() and col.data.dtype == np.int32
    assert [CC.numpy_classes(a) for a in arrays] == [[int(h[f]) for f in ("idle", "served", "unserved")] for h in col.headers]
    assert col.offsets.tolist() == np.concatenate([[0], np.cumsum([c.nUE for c in cfgs])[:-1]]).tolist()
    tm = eng.timing()
    assert tm.columns_ms > 0 and (tm.pick_ms, tm.xtab_ms, tm.trace_ms, tm.summary_ms, tm.dist_ms, tm.timeline_ms, tm.sojourn_ms) == (0, 0, 0, 0, 0, 0, 0)
    return res, logs, col


@pytest.mark.parametrize("rng", ["glibc", "philox"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_columns_equal_logs_numpy_and_oracle(pkg, ob, eng, kernel, rng):
    for k, v in KERNELS[kernel].items():
        eng.set(k, v)
    cfgs = trial_cfgs(pkg, pkg.RNG_GLIBC if rng == "glibc" else pkg.RNG_PHILOX)
    oracle = [oracle_trial(ob, c) for c in cfgs]
    for fields in SPECS:
        res, logs, col = run_checked(pkg, eng, cfgs, fields)
        assert np.array_equal(col.data, numpy_of(pkg, cfgs, [a for a, _ in oracle], [E for _, E in oracle], col))
    assert (col.trial(3) == -1).sum() >= 3 * 300 and np.array_equal(col.data[0], col.data[2]) and np.array_equal(col.data[1], col.data[4])  # (REPEATED; the cut trial: everybody idle)


def test_trials_around_the_tile_in_one_call(pkg, eng):
    """8191, 8192 and 8193 UEs: an odd offset follows a tile edge, and the last trial has a second tile of one UE."""
    tile = pkg.columns_tile_ues()
    cfgs = [pkg.make_cfg(tile + d, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s, (d, v) in enumerate(((-1, 0), (0, 1), (1, 0)))]
    for fields in (MENU, RAW, ["age"]):
        _, _, col = run_checked(pkg, eng, cfgs, fields)
        assert col.offsets.tolist() == [0, tile - 1, 2 * tile - 1]


def test_with_and_without_logs_and_next_to_plain_run_trials(pkg, eng):
    cfgs = trial_cfgs(pkg, pkg.RNG_PHILOX)
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    assert eng.timing().columns_ms == 0
    res1, logs1, col1 = run_checked(pkg, eng, cfgs, MENU)
    res2, nologs, col2 = eng.run_trials_columns(cfgs, MENU)  # no host logs
    assert nologs == [None] * len(cfgs) and eng.timing().columns_ms > 0
    res3, some, col3 = eng.run_trials_columns(cfgs, MENU, want_logs=[1])
    assert some[0] is None and bytes(some[1]) == bytes(logs0[1])
    assert same(col2, col1) and same(col3, col1)
    for res in (res1, res2, res3):
        assert [bytes(r) for r in res] == [bytes(r) for r in res0]
    assert all(bytes(a) == bytes(b) for a, b in zip(logs1, logs0))
    eng.run_trials(cfgs)
    assert eng.timing().columns_ms == 0
    _, _, xt = eng.run_trials_xtab(cfgs)  # the kinds share one device buffer: columns after a cross-tabulation, and its class counts
    assert eng.timing().columns_ms == 0 and eng.timing().xtab_ms > 0
    _, _, col4 = eng.run_trials_columns(cfgs, MENU)
    assert same(col4, col1) and all(col1.headers[f].tolist() == xt.scalars[f].tolist() for f in ("idle", "served", "unserved"))


def undisturbed_then(pkg, cfgs, disturb, fields):
    """The columns of the call as it is and of the same call after `disturb(engine)`, each on an engine of its own; both checked against their logs."""
    out = []
    for fn in (None, disturb):
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, col = run_checked(pkg, e, cfgs, fields)
            out.append((col, e.timing()))
        finally:
            e.close()
    (a, t0), (b, t1) = out
    assert same(a, b)
    return t0, t1


def test_written_once_calendar_rerun(pkg):
    cases = [(3000, {}), (8000, dict(nGrantUL=3)), (12000, dict(nGrantUL=2))]  # the shapes of test_calendar_cap_rerun_is_exact: lists of 64 entries fill
    cfgs = [pkg.make_cfg(n, variant=1, rng_mode=pkg.RNG_PHILOX, seed=s, **kw) for s in (0, 1) for n, kw in cases]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("calendar_cap", 64), ["state", "age", "raw:preambleTxCounter", "sojourn"])
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1.launches > t0.launches


def test_written_once_mem_budget_split(pkg):
    cfgs = [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(8) for v in (0, 1) for n in (3000, 6000)]
    t0, t1 = undisturbed_then(pkg, cfgs, lambda e: e.set("mem_budget_mb", 64), MENU)
    assert t1.launches >= 2 and t1.launches > t0.launches


def test_refusals_and_rows_behind_the_sum_keep_a_sentinel(pkg, eng):
    cfgs = trial_cfgs(pkg, pkg.RNG_PHILOX)[:3]
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c: refused before anything is launched
        eng.run_trials_columns(cfgs + [pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1)], MENU)
    assert ei.value.status == -2
    for fields in ([], ["one"] * 17, [9], [32], [-1]):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_columns(cfgs, fields)
        assert ei.value.status == -1, fields
    # the C entry point with an engine: a capacity one short is refused and nothing is written; with room to spare the rows behind the sum are not touched
    L = pkg.lib()
    n, rows = len(cfgs), sum(c.nUE for c in cfgs)
    arr, res, hdr = (pkg.PrachCfg * n)(*cfgs), (pkg.PrachResult * n)(), (pkg.PrachColumns * n)()
    sp, ids = pkg.columns_spec(REPEATED)
    sentinel = 0x1234567
    out = np.full((len(ids), rows + 7), sentinel, dtype=np.int32)
    assert L.prach_run_trials_columns(eng._h, arr, n, res, None, C.byref(sp), hdr, out.ctypes.data, rows - 1) == -1
    assert L.prach_run_trials_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, out.ctypes.data, rows + 7) == -1  # host memory is no device destination
    bad, _ = pkg.columns_spec(["one"])
    bad.reserved[2] = 1
    assert L.prach_run_trials_columns(eng._h, arr, n, res, None, C.byref(bad), hdr, out.ctypes.data, rows + 7) == -1
    assert (out == sentinel).all() and bytes(hdr) == bytes(C.sizeof(hdr))
    assert L.prach_run_trials_columns(eng._h, arr, n, res, None, C.byref(sp), hdr, out.ctypes.data, rows + 7) == 0
    _, _, col = eng.run_trials_columns(cfgs, REPEATED)  # ... and the engine goes on
    assert np.array_equal(out[:, :rows], col.data) and (out[:, rows:] == sentinel).all() and (col.data != sentinel).all()
    assert [h.offset for h in hdr] == col.offsets.tolist() and [h.served for h in hdr] == col.headers["served"].tolist()


@pytest.mark.parametrize("mode", ["torch_first", "reversed"])
def test_device_destination_in_a_child_process(pkg, mode):
    """torch first: the kernel writes straight into a torch tensor (tests/tools/gpu_columns_device_child.py has the checks).  The library first: torch brings
    a second HIP runtime, and the binding refuses device=True saying so."""
    p = subprocess.run([sys.executable, CHILD, mode], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.returncode, p.stdout[-500:], p.stderr[-3000:])
