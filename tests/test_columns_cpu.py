"""Host side of the per-UE columns (include/prach.h, prach_columns_*): the definition prach::columns_kernel must equal, against the numpy restatement of the
menu (xtab_ref.values) and the log words themselves over the oracle's UEs, a literal block, the struct sizes and the refusals of prach_run_trials_columns
that need no device.  No GPU."""
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
import xtab_ref as X  # noqa: E402

# nUE <= 3000, both programs: the trials of tests/test_gpu_pick.py (one with restarts, one Uniform, one cut after 3 subframes, odd sizes)
CASES = [(3000, dict(variant=0, seed=1)), (2000, dict(variant=1, seed=2, maxMsg2TxCount=3)), (500, dict(variant=0, seed=3, uniform=1)), (300, dict(variant=0, seed=4, max_steps=3)),
         (1, dict(variant=1, seed=5)), (65, dict(variant=0, seed=6)), (1025, dict(variant=1, seed=7)), (3000, dict(variant=0, seed=8, max_steps=2500))]
CUT, UNIFORM, HALF = 3, 2, 7  # cut after 3 subframes: everybody is idle; cut after 2500: idle, served and unserved UEs
RAW_NAMES = ["raw:" + n for n in ("idx", "timer", "active", "txTime", "firstTxTime", "secondTxTime", "nowBackoff", "preamble", "preambleChange", "rarWindow", "maxRarCounter",
                                  "preambleTxCounter", "msg2Flag", "connectionRequest", "msg4Flag", "failCount")]


@pytest.fixture(scope="module")
def trials(pkg, ob):
    """(product cfg, oracle result, oracle UEs as int32 [nUE, 16], the oracle's arrival schedule) per case, in both RNG modes, computed once."""
    out = []
    for rng in (pkg.RNG_PHILOX, pkg.RNG_GLIBC):
        for n, kw in CASES:
            c = pkg.make_cfg(n, rng_mode=rng, **kw)
            oc = T.oracle_cfg(ob, c)
            res, ues = ob.run_trial(oc, ob.Rng(c.rng_mode, c.seed))
            out.append((c, res, T.as_array(ues).copy(), ob.arrival_schedule(oc)[0]))
    return out


def call(pkg, trials, fields):
    return pkg.columns_from_logs([c for c, _, _, _ in trials], [r.steps for _, r, _, _ in trials], [a for _, _, a, _ in trials], fields)


def test_menu_fields_equal_xtab_ref_and_raw_fields_the_log_words(pkg, trials):
    col = call(pkg, trials, list(pkg.XTAB_FIELD_NAMES) + RAW_NAMES[:7])
    raw = call(pkg, trials, RAW_NAMES)
    assert col.fields[:9] == pkg.XTAB_FIELD_NAMES and raw.fields == tuple(RAW_NAMES) and col.data.shape == (16, sum(n for n, _ in CASES) * 2) and col.data.dtype == np.int32
    assert col.offsets.tolist() == np.concatenate([[0], np.cumsum([c.nUE for c, _, _, _ in trials])[:-1]]).tolist()
    for k, (c, res, a, sched) in enumerate(trials):
        E = min(res.steps, res.maxTime)
        for f in range(9):
            v = X.values(f, a, sched, c.accessTime, E)
            assert np.array_equal(col.trial(k)[f], np.where(v < 0, -1, v)), (k, f)
        assert np.array_equal(col.trial(k), CC.numpy_columns(a, sched, c.accessTime, E, col.field_ids))
        assert np.array_equal(raw.trial(k), a.T) and np.array_equal(col.trial(k)[9:], a.T[:7])
    # what the trials reach: undefined values of every kind, and raw and menu timers that differ for the idle UEs
    assert trials[CUT][1].steps == 3 and (col.trial(CUT)[1:8] == -1).all() and (col.trial(CUT)[X.STATE] == 0).all() and (col.trial(CUT)[X.ONE] == 0).all()
    k = HALF
    c, res, a, _ = trials[k]
    idle = a[:, T.ACTIVE] == -1
    assert res.steps == 2500 and 0 < idle.sum() < c.nUE and (col.trial(k)[X.ARRIVAL][idle] == -1).all() and (col.trial(k)[X.AGE][~idle] >= 0).all()
    assert (col.trial(k)[X.STATE][idle] == 0).all() and {0, 1} <= set(col.trial(k)[X.STATE].tolist()) and col.trial(k)[X.STATE].max() >= 2 and ((col.trial(k)[X.SOJOURN] == -1) & ~idle).any()
    assert np.array_equal(col.column("arrival"), col.data[1]) and col.column("raw:idx").base is not None  # views
    assert trials[UNIFORM][0].uniform == 1 and (np.diff(col.trial(UNIFORM)[X.ARRIVAL]) >= 0).all() and col.trial(UNIFORM)[X.ARRIVAL].min() == 0


def test_timer_and_raw_timer_differ_for_idle_ues(pkg, trials):
    two = call(pkg, trials[HALF:HALF + 1], ["timer", "raw:timer", "timer"])  # (a field may be named twice)
    a = trials[HALF][2]
    idle = a[:, T.ACTIVE] == -1
    assert 0 < idle.sum() < len(a)
    assert np.array_equal(two.data[1], a[:, T.TIMER]) and np.array_equal(two.data[0], two.data[2])
    assert (two.data[0][idle] == -1).all() and np.array_equal(two.data[0][~idle], a[~idle, T.TIMER])
    # an idle UE that logs a timer of its own: the menu says UNDEFINED, the raw word says what was logged
    b = a.copy()
    b[idle, T.TIMER] = 77
    two = pkg.columns_from_logs([trials[HALF][0]], [2500], [b], ["timer", "raw:timer"])
    assert (two.data[0][idle] == -1).all() and (two.data[1][idle] == 77).all()


def test_class_counts_equal_xtab_ref_classes(pkg, trials):
    col = call(pkg, trials, ["one"])
    for k, (c, _, a, _) in enumerate(trials):
        cls = X.classes(a)
        h = col.headers[k]
        assert [int(h["idle"]), int(h["served"]), int(h["unserved"])] == [int((cls == b).sum()) for b in (X.IDLE, X.SERVED, X.UNSERVED)] == CC.numpy_classes(a)
        assert int(h["idle"]) + int(h["served"]) + int(h["unserved"]) == c.nUE == int(h["nUE"]) and int(h["status"]) == 0


def test_literal_block(pkg):
    """Six UEs written down by hand, one per class and state: Beta.c, accessTime 5, the arrivals a(i) those of the product's own schedule."""
    c = pkg.make_cfg(6, variant=0, rng_mode=pkg.RNG_PHILOX, seed=0)
    sched = pkg.arrival_schedule(c)[0]
    at = [c.accessTime * int(np.searchsorted(sched, i, side="right")) for i in range(6)]
    a = np.zeros((6, 16), dtype=np.int32)
    # words 0-3 are idx, timer, active, txTime; 6 nowBackoff, 11 preambleTxCounter, 13 connectionRequest, 14 msg4Flag, 15 failCount
    a[0, :4] = (0, -1, -1, -1)  # idle
    a[1, :4] = (1, 40, 0, at[1] + 34); a[1, 11] = 3; a[1, 14] = 1; a[1, 15] = 2  # served
    a[2, :4] = (2, 9, 1, 0); a[2, 6] = 4; a[2, 11] = 1  # in a backoff
    a[3, :4] = (3, 12, 1, 0); a[3, 6] = 0; a[3, 11] = 2  # in a RAR window
    a[4, :4] = (4, 20, 2, 0); a[4, 13] = 47  # Msg3 pending
    a[5, :4] = (5, 21, 2, 0); a[5, 13] = 48  # waiting out the Msg3 timeout
    E = at[5] + 100
    col = pkg.columns_from_logs([c], [E], [a], list(pkg.XTAB_FIELD_NAMES) + ["raw:timer", "raw:connectionRequest"])
    assert col.data.tolist() == [
        [0, 0, 0, 0, 0, 0],                                                            # one
        [-1] + at[1:],                                                                 # arrival
        [-1, 40, -1, -1, -1, -1],                                                      # sojourn = txTime + 6 - a
        [-1, at[1] + 40, -1, -1, -1, -1],                                              # completion
        [-1, 40, 9, 12, 20, 21],                                                       # timer
        [-1, 3, 1, 2, 0, 0],                                                           # ptc
        [-1, 2, 0, 0, 0, 0],                                                           # failcount
        [-1] + [E - t for t in at[1:]],                                                # age
        [0, 1, 2, 3, 4, 5],                                                            # state
        [-1, 40, 9, 12, 20, 21],                                                       # raw:timer
        [0, 0, 0, 0, 47, 48]]                                                          # raw:connectionRequest
    assert [int(col.headers[n][0]) for n in ("idle", "served", "unserved")] == [1, 1, 4]
    short = pkg.columns_from_logs([c], [at[4]], [a], ["age"])  # E below an arrival: that UE's AGE is undefined
    assert at[5] > at[4] and short.data[0].tolist() == [-1] + [at[4] - t for t in at[1:5]] + [-1]


def test_refusals_that_need_no_device(pkg):
    L = pkg.lib()
    cfgs = (pkg.PrachCfg * 2)(pkg.make_cfg(100, rng_mode=pkg.RNG_PHILOX), pkg.make_cfg(50, rng_mode=pkg.RNG_PHILOX))
    res = (pkg.PrachResult * 2)()
    hdr = (pkg.PrachColumns * 2)()
    out = np.full(16 * 200, 7, dtype=np.int32)
    good, _ = pkg.columns_spec(["arrival", "raw:timer"])

    def both(spec, h, dst, cap, c=cfgs):
        rc = [fn(None, c, 2, res, None, spec, h, dst, cap) for fn in (L.prach_run_trials_columns, L.prach_run_trials_columns_device)]
        assert rc[0] == rc[1]
        return rc[0]

    assert both(C.byref(good), hdr, out.ctypes.data, 150) == -1  # (everything is in order but the engine: the engine is asked for last)
    assert both(None, hdr, out.ctypes.data, 150) == -1 and both(C.byref(good), None, out.ctypes.data, 150) == -1 and both(C.byref(good), hdr, None, 150) == -1
    for fields in ([], ["one"] * 17, [9], [15], [32], [-1]):
        sp, _ = pkg.columns_spec(fields)
        assert both(C.byref(sp), hdr, out.ctypes.data, 200) == -1, fields
    for w in range(3):
        sp, _ = pkg.columns_spec(["one"])
        sp.reserved[w] = 1
        assert both(C.byref(sp), hdr, out.ctypes.data, 200) == -1
    assert both(C.byref(good), hdr, out.ctypes.data, 149) == -1  # rows_cap one short of the sum of nUE
    noma = (pkg.PrachCfg * 2)(pkg.make_cfg(100, rng_mode=pkg.RNG_PHILOX), pkg.make_cfg(50, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX))
    assert both(C.byref(good), hdr, out.ctypes.data, 150, noma) == -2
    sp16, _ = pkg.columns_spec(["one"] * 16)
    assert both(C.byref(sp16), hdr, out.ctypes.data, pkg.COL_MAX_WORDS // 16 + 1) == -2 and both(C.byref(good), hdr, out.ctypes.data, pkg.COL_MAX_WORDS + 1) == -2
    assert both(C.byref(sp16), hdr, out.ctypes.data, pkg.COL_MAX_WORDS // 16) == -1  # (within the limit: only the engine is missing)
    assert 16 * 55_000_000 <= pkg.COL_MAX_WORDS  # the 1000-trial grid with 16 columns fits
    assert (out == 7).all() and bytes(hdr) == bytes(C.sizeof(hdr))  # nothing was written
    # the host definition's own refusals
    a = np.zeros((100, 16), dtype=np.int32)
    buf = np.zeros(200, dtype=np.int32)
    lp = a.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
    assert L.prach_columns_from_logs(C.byref(good), C.byref(cfgs[0]), 10, lp, 100, buf.ctypes.data, 100) == 0
    assert L.prach_columns_from_logs(C.byref(good), C.byref(cfgs[0]), 10, lp, 100, buf.ctypes.data, 99) == -1
    assert L.prach_columns_from_logs(C.byref(good), C.byref(cfgs[0]), 10, lp, 99, buf.ctypes.data, 100) == -1
    assert L.prach_columns_from_logs(None, C.byref(cfgs[0]), 10, lp, 100, buf.ctypes.data, 100) == -1
    assert L.prach_columns_from_logs(C.byref(good), C.byref(noma[1]), 10, lp, 50, buf.ctypes.data, 100) == -2
    with pytest.raises(ValueError):
        pkg.columns_spec(["raw:nosuchword"])
    with pytest.raises(ValueError):
        pkg.columns_spec(["nosuchfield"])


def test_struct_sizes_agree(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "prach.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %llu\\n", sizeof(prach_columns_spec),'
                   ' sizeof(prach_columns), offsetof(prach_columns, offset), offsetof(prach_columns, idle), sizeof(prach_timing), offsetof(prach_timing, columns_ms),'
                   ' offsetof(prach_timing, pick_ms), PRACH_COL_MAX, PRACH_COL_RAW, (unsigned long long)PRACH_COL_MAX_WORDS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert sizes == [C.sizeof(pkg.PrachColumnsSpec), C.sizeof(pkg.PrachColumns), pkg.PrachColumns.offset.offset, pkg.PrachColumns.idle.offset, C.sizeof(pkg.PrachTiming),
                     pkg.PrachTiming.columns_ms.offset, pkg.PrachTiming.pick_ms.offset, pkg.COL_MAX, pkg.COL_RAW, pkg.COL_MAX_WORDS]
    assert sizes[:4] == [80, 32, 8, 16] and sizes[5] + 8 == sizes[6] and pkg.columns_header_dtype().itemsize == 32
    assert pkg.PrachTiming._fields_[-1][0] == "sojourn_ms" and pkg.PrachTiming.sojourn_ms.offset + 8 == sizes[4]  # sojourn_ms stays the last member
    for sym in ("prach_run_trials_columns", "prach_run_trials_columns_device", "prach_columns_from_logs", "prach_columns_tile_ues"):
        assert sym in pkg.EXPORTS
    assert pkg.columns_tile_ues() == CC.TILE
