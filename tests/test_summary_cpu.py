"""Host side of the per-trial summary (include/prach.h, prach_summary_*): the definition prach::summary_kernel must equal, against a numpy restatement
(np.sort plus the integer rank rule) over the oracle's UEs and against the timeline, dist and sojourn definitions already here; the statistics across
trials against np.mean / np.std, the CSV text, the gather of dist.py and the argument checks of prach_run_trials_summary that need no device.  No GPU."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import summary_ref as R  # noqa: E402
import timeline_ref as T  # noqa: E402

# Beta.c 300 UEs; RandomAccessWithNOMA 2000 UEs with three Msg2 retransmissions (UEs start over); Uniform traffic 500 UEs; a trial cut after 3 subframes
CASES = [(300, dict(variant=0, seed=1)), (2000, dict(variant=1, seed=2, maxMsg2TxCount=3)), (500, dict(variant=0, seed=3, uniform=1)),
         (300, dict(variant=0, seed=4, max_steps=3))]
RESTARTS, UNIFORM, NOBODY = 1, 2, 3
LEVELS = (1, 250, 500, 501, 900, 950, 990, 1000)


@pytest.fixture(scope="module")
def trials(pkg, ob):
    """(product cfg, oracle result, oracle UEs as int32 [nUE, 16], the oracle's arrival schedule) per case, computed once."""
    out = []
    for n, kw in CASES:
        c = pkg.make_cfg(n, **dict(dict(rng_mode=pkg.RNG_PHILOX), **kw))
        oc = T.oracle_cfg(ob, c)
        res, ues = ob.run_trial(oc, ob.Rng(c.rng_mode, c.seed))
        out.append((c, res, T.as_array(ues).copy(), ob.arrival_schedule(oc)[0]))
    return out


@pytest.mark.parametrize("levels", [LEVELS, (500, 950, 990), (1000,)], ids=lambda l: "-".join(map(str, l)))
def test_from_logs_equals_numpy_on_oracle_ues(pkg, trials, levels):
    sm = pkg.summary_from_logs([t[0] for t in trials], [t[2] for t in trials], levels)
    R.check_rows(sm.rows, [R.trial_row(a, sched, c.accessTime, levels) for c, _, a, sched in trials])
    for (c, res, a, _), r in zip(trials, sm.rows):
        assert int(r["nUE"]) == c.nUE and int(r["arrived"]) == res.activeCheck and int(r["success"]) == res.nSuccessUE
        assert int(r["timer_sum"]) == res.sumTimer and int(r["ptc_sum"]) == res.preambleTxCount
    assert int(sm.rows[RESTARTS]["restarted"]) > 0 and int(sm.rows[UNIFORM]["sojourn_max"]) >= 0
    nobody = sm.rows[NOBODY]
    assert int(nobody["success"]) == 0 and int(nobody["status"]) == 0 and (nobody["q"] == -1).all()
    assert [int(nobody[f]) for f in ("sojourn_max", "timer_max", "ptc_max", "sojourn_sum", "timer_sum", "ptc_sum")] == [-1, -1, -1, 0, 0, 0]
    assert (sm.rows["q"][:, :, len(levels):] == -1).all()  # unused levels


def test_cross_checks_against_timeline_dist_and_sojourn(pkg, trials):
    cfgs, logs = [t[0] for t in trials], [t[2] for t in trials]
    sm = pkg.summary_from_logs(cfgs, logs, (500,))
    tl = pkg.timeline_from_logs(cfgs, logs, 16, 5000)  # one group per trial
    d = pkg.dist_from_logs(logs, 4096, 16)
    sj = pkg.sojourn_from_logs(cfgs, logs, 1, 70000, 16384, 1)  # pooled rows, 1 ms bins: Beta sojourns fit; Uniform ones may not
    for g, r in enumerate(sm.rows):
        for f in ("arrived", "success", "restarted", "sojourn_sum", "timer_sum"):
            assert int(r[f]) == int(tl.scalars[f][g]), (g, f)
        assert int(r["ptc_sum"]) == int(d.ptc_sum[g]) and int(r["timer_max"]) == int(d.delay_max[g]) and int(r["timer_sum"]) == int(d.delay_sum[g])
        assert int(r["sojourn_max"]) == int(sj.scalars["sojourn_max"][g])
        if int(sj.scalars["delay_overflow"][g]) == 0:
            assert int(r["q"][0, 0]) == sj.quantile(g, -1, 0.5), g  # level 500 is ceil(0.5 n): the one level at which the two rules coincide
    assert int(sj.scalars["delay_overflow"][0]) == 0 and int(sm.rows[0]["q"][0, 0]) > 0


def test_rank_rule(pkg):
    """The rule at n = 999, 1000, 1001 for levels 1, 500, 1000, on values that name their rank (the k-th smallest sojourn is 7 k)."""
    want = {999: (1, 500, 999), 1000: (1, 500, 1000), 1001: (2, 501, 1001)}
    for n, ranks in want.items():
        assert tuple(R.rank(n, m) for m in (1, 500, 1000)) == ranks
        c = pkg.make_cfg(n, variant=0, rng_mode=pkg.RNG_PHILOX, seed=0)
        at = c.accessTime * np.searchsorted(np.asarray(pkg.arrival_schedule(c)[0]), np.arange(n), side="right")
        perm = np.random.default_rng(n).permutation(n) + 1
        a = np.zeros((n, 16), dtype=np.int32)
        a[:, T.FLAG], a[:, T.TXTIME], a[:, T.TIMER], a[:, R.PTC] = 1, at + 7 * perm - 6, 3 * perm[::-1], (perm % 50) + 1
        row = pkg.summary_from_logs([c], [a], (1, 500, 1000)).rows[0]
        assert row["q"][0, :3].tolist() == [7 * k for k in ranks] and row["q"][1, :3].tolist() == [3 * k for k in ranks]
        assert row["q"][2, :3].tolist() == [int(np.sort(perm % 50 + 1)[k - 1]) for k in ranks]
        R.check_rows([row], [R.trial_row(a, pkg.arrival_schedule(c)[0], c.accessTime, (1, 500, 1000))])
    assert R.rank(1, 1) == 1 and R.rank(3, 1000) == 3 and R.rank(2 ** 24, 999) == 16760439  # 64-bit product: 2^24 x 999 > 2^31


def _rows(pkg, n, seed, levels=(500, 990)):
    """Synthetic rows: plausible integers, some trials failed, some without a successful UE."""
    rng = np.random.default_rng(seed)
    sm = pkg.Summary(n, levels)
    r = sm.rows
    r["nUE"] = rng.integers(100, 5000, n)
    r["success"] = (r["nUE"] * rng.random(n)).astype(np.int32)
    r["success"][rng.random(n) < 0.1] = 0
    r["status"] = np.where(rng.random(n) < 0.1, -3, 0)
    r["arrived"] = r["nUE"]
    r["restarted"] = (r["success"] * rng.random(n)).astype(np.int32)
    for f in ("sojourn_sum", "timer_sum", "ptc_sum"):
        r[f] = r["success"].astype(np.int64) * rng.integers(1, 3000, n)
    r["q"] = -1
    r["q"][:, :, :len(levels)] = rng.integers(0, 60000, (n, 3, len(levels)))
    return sm


def test_stats_against_numpy(pkg):
    """Relative 1e-9: n eps with a wide margin for n <= 1000 (eps = 2.2e-16; two-pass sums of n terms)."""
    for n, ng, seed in ((1000, 1, 0), (300, 7, 1), (40, 40, 2), (5, 2, 3)):
        sm = _rows(pkg, n, seed)
        groups = [k % ng for k in range(n)]
        got = sm.stats(groups, ng)
        assert got.shape == (ng, 5 + 3 * 2) and sm.metric_names()[5:] == ["sojourn_p500", "sojourn_p990", "timer_p500", "timer_p990", "ptx_p500", "ptx_p990"]
        ref = R.stats_ref(sm.rows, sm.permille, groups, ng)
        for (g, m), want in ref.items():
            have = got[g, m]
            assert int(have["n"]) == want[0], (g, m)
            for f, w in zip(("mean", "sd", "sem", "min", "max"), want[1:]):
                assert float(have[f]) == pytest.approx(w, rel=1e-9, abs=0.0), (n, g, m, f)
        if ng == 1:  # no group table: one group
            assert sm.stats().tobytes() == got.tobytes()
    # n = 1: no spread; n = 0: everything 0; a failed row counts nowhere, a row without a successful UE in success_ratio only
    sm = pkg.Summary(3, (500,))
    sm.rows["nUE"], sm.rows["success"], sm.rows["status"] = [10, 10, 10], [0, 4, 9], [0, 0, -3]
    sm.rows["q"][:, :, 0] = [[0] * 3, [8, 9, 10], [99] * 3]
    st = sm.stats()
    assert [int(x) for x in st[0]["n"]] == [2, 1, 1, 1, 1, 1, 1, 1] and float(st[0, 0]["mean"]) == 0.2 and float(st[0, 5]["mean"]) == 8.0
    assert float(st[0, 5]["sd"]) == 0.0 and float(st[0, 5]["sem"]) == 0.0 and float(st[0, 0]["sd"]) == pytest.approx(np.std([0.0, 0.4], ddof=1), rel=1e-12)
    empty = pkg.Summary(2, (500,))
    empty.rows["status"] = -3
    assert not np.frombuffer(empty.stats([0, 1], 3).tobytes(), dtype=np.uint8).any()
    for bad in (dict(groups=[0, 3], ngroups=3), dict(groups=[0, -1], ngroups=3)):
        with pytest.raises(pkg.PrachError) as ei:
            empty.stats(**bad)
        assert ei.value.status == -1
    for levels in ((), (0,), (1001,), tuple(range(1, 10))):
        with pytest.raises(pkg.PrachError) as ei:
            pkg.Summary(2, levels).stats()
        assert ei.value.status == -1


def test_csv_is_pinned(pkg):
    sm = pkg.Summary(4, (500, 1000))
    r = sm.rows
    r["nUE"], r["success"], r["restarted"] = [10, 10, 20, 20], [5, 10, 0, 20], [1, 0, 0, 5]
    r["sojourn_sum"], r["timer_sum"], r["ptc_sum"] = [100, 300, 0, 10], [50, 100, 0, 10], [5, 15, 0, 30]
    r["q"] = -1
    r["q"][:, :, :2] = [[[20, 30], [10, 12], [1, 2]], [[30, 70], [10, 20], [1, 3]], [[-1, -1]] * 3, [[7, 7], [7, 7], [7, 7]]]
    text = pkg.summary_csv(sm, groups=[0, 0, 1, 1], labels=["10", "20"])
    assert text == (b"10,success_ratio,2,0.75,0.353553391,0.25,0.5,1\n"
                    b"10,restart_ratio,2,0.1,0.141421356,0.1,0,0.2\n"
                    b"10,sojourn_mean,2,25,7.07106781,5,20,30\n"
                    b"10,timer_mean,2,10,0,0,10,10\n"
                    b"10,ptx_mean,2,1.25,0.353553391,0.25,1,1.5\n"
                    b"10,sojourn_p500,2,25,7.07106781,5,20,30\n"
                    b"10,sojourn_p1000,2,50,28.2842712,20,30,70\n"
                    b"10,timer_p500,2,10,0,0,10,10\n"
                    b"10,timer_p1000,2,16,5.65685425,4,12,20\n"
                    b"10,ptx_p500,2,1,0,0,1,1\n"
                    b"10,ptx_p1000,2,2.5,0.707106781,0.5,2,3\n"
                    b"20,success_ratio,2,0.5,0.707106781,0.5,0,1\n"
                    b"20,restart_ratio,1,0.25,0,0,0.25,0.25\n"
                    b"20,sojourn_mean,1,0.5,0,0,0.5,0.5\n"
                    b"20,timer_mean,1,0.5,0,0,0.5,0.5\n"
                    b"20,ptx_mean,1,1.5,0,0,1.5,1.5\n"
                    b"20,sojourn_p500,1,7,0,0,7,7\n"
                    b"20,sojourn_p1000,1,7,0,0,7,7\n"
                    b"20,timer_p500,1,7,0,0,7,7\n"
                    b"20,timer_p1000,1,7,0,0,7,7\n"
                    b"20,ptx_p500,1,7,0,0,7,7\n"
                    b"20,ptx_p1000,1,7,0,0,7,7\n")
    sp, st = sm.spec(), sm.stats()
    args = (C.byref(sp), st[0].ctypes.data_as(C.POINTER(pkg.PrachStat)), b"x")
    need = pkg.lib().prach_summary_format_csv(*args, None, 0)
    small = C.create_string_buffer(b"y" * 40, 41)
    assert need > 40 and pkg.lib().prach_summary_format_csv(*args, small, 40) == need and small.value == b""  # does not fit: the length only


def test_refusals_and_argument_errors_need_no_device(pkg, trials):
    c, _, a, _ = trials[0]
    for levels in ((), (0,), (1001,), tuple(range(1, 10))):
        with pytest.raises(pkg.PrachError) as ei:
            pkg.summary_from_logs([c], [a], levels)
        assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # the log is not this config's
        pkg.summary_from_logs([c], [a[:-1]], (500,))
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c logs no trace of a cycle start
        pkg.summary_from_logs([pkg.make_cfg(c.nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX)], [a], (500,))
    assert ei.value.status == -2
    ok = np.flatnonzero(a[:, T.FLAG] == 1)
    for col, val in ((T.TIMER, -3), (T.TXTIME, -100)):  # a successful UE with a negative timer / a completion before its arrival: refused, the row untouched
        b = a.copy()
        b[ok[len(ok) // 2], col] = val
        sm = pkg.Summary(1, (500,))
        sm.rows["arrived"] = 12345
        sp = sm.spec()
        ptr = b.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
        assert pkg.lib().prach_summary_from_logs(C.byref(sp), C.byref(c), ptr, c.nUE, sm._rows_ptr()) == -1 and int(sm.rows["arrived"][0]) == 12345
    # prach_run_trials_summary: spec and variants are judged before the engine is looked at
    L = pkg.lib()
    n = 3
    res = (pkg.PrachResult * n)()
    rows = (pkg.PrachTrialSummary * n)()

    def call(nq=3, levels=(500, 950, 990), reserved=(0, 0, 0), rr=rows, spec=True, nn=n, variants=(0, 1, 0)):
        cfgs = (pkg.PrachCfg * n)(*[pkg.make_cfg(100, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s, v in enumerate(variants)])
        sp = pkg.PrachSummarySpec()
        sp.nq = nq
        for l, m in enumerate(levels):
            sp.permille[l] = m
        for l, m in enumerate(reserved):
            sp.reserved[l] = m
        return L.prach_run_trials_summary(None, cfgs, nn, res, None, C.byref(sp) if spec else None, rr)

    assert call() == -1  # everything in order but the engine
    assert call(variants=(0, 2, 1)) == -2  # a NOMA.c trial: refused before anything could be launched
    for bad in (dict(nq=0), dict(nq=9), dict(levels=(500, 0, 990)), dict(levels=(500, 950, 1001)), dict(reserved=(0, 0, 1)), dict(reserved=(1, 0, 0)), dict(rr=None),
                dict(spec=False), dict(nn=0)):
        assert call(**bad) == -1, bad
    assert call(variants=(2, 2, 2), nq=0) == -1  # a bad spec in a request with a NOMA.c trial is an argument error
    assert pkg.summary_max_value() == 65535
    assert C.sizeof(pkg.PrachTrialSummary) == 160 == pkg.summary_row_dtype().itemsize and C.sizeof(pkg.PrachStat) == 48 == pkg.summary_stat_dtype().itemsize
    assert "summary_ms" in [f for f, _ in pkg.PrachTiming._fields_] and C.sizeof(pkg.PrachTiming) % 8 == 0
    for sym in ("prach_run_trials_summary", "prach_summary_from_logs", "prach_summary_stats", "prach_summary_format_csv", "prach_summary_max_value"):
        assert sym in pkg.EXPORTS


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same_rows(x, y):
    """Field by field (the padding of a row means nothing)."""
    return len(x) == len(y) and all(np.array_equal(x[f], y[f]) for f in y.dtype.names)


GATHER_N = 11  # trials of the grid: rank 0 holds the odd ones, in descending order; rank 1 the even ones


def _gather_worker(rank, world, port, q):
    import importlib
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    distmod = importlib.import_module("nr_randomaccess_amd.dist")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    every = _rows(pkg, GATHER_N, 5).rows
    mine = [k for k in range(GATHER_N) if k % 2 != rank][::-1 if rank == 0 else 1]
    got = distmod.gather_summary_rows(every[mine], mine, dst=0)
    q.put((rank, None if got is None else got.tobytes()))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_summary_rows_two_ranks_gloo(pkg):
    import importlib
    distmod = importlib.import_module("nr_randomaccess_amd.dist")
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    every = _rows(pkg, GATHER_N, 5).rows
    assert outs[1] is None and _same_rows(np.frombuffer(outs[0], dtype=every.dtype), every)  # rank 0 holds every row, in trial order
    # without a process group: the rows in trial order
    order = np.random.default_rng(0).permutation(GATHER_N)
    assert _same_rows(distmod.gather_summary_rows(every[order], order), every)
    with pytest.raises(ValueError):
        distmod.gather_summary_rows(every[:3], [0, 1])
