"""Host side of the timelines per trial group (include/prach.h, prach_timeline_*): the definition prach::timeline_kernel must equal, against a numpy
restatement over the oracle's UEs and against the invariants that tie it to the oracle's own results; the merge, the CSV text, the all-reduce of
dist.py and the argument checks of prach_run_trials_timeline that need no device.  No GPU."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import timeline_ref as T  # noqa: E402

# (nUE, overrides): the trials of the GPU suite's window cases, its overloaded trial (most successful UEs started over) and its truncated trial
CASES = [(8000, dict(variant=1, seed=9)), (1000, dict(variant=0, seed=1, uniform=1)), (3000, dict(variant=1, seed=2, accessTime=1)),
         (3000, dict(variant=0, seed=3, accessTime=7)), (20000, dict(variant=1, seed=7, maxMsg2TxCount=3)), (8000, dict(variant=1, seed=9, max_steps=2500)),
         (4097, dict(variant=0, seed=11, rng_mode=0))]


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


def horizon(c, width):
    return -(-((60000 if c.uniform else 10000) + 6) // width)


@pytest.mark.parametrize("width", [1, 5, 7])
def test_accumulate_logs_equals_numpy_on_oracle_ues(pkg, trials, width):
    for c, res, a, sched in trials:
        for bins in (horizon(c, width), max(1, 1500 // width), 1):  # the whole horizon; cut short of it; one bin
            host = pkg.timeline_from_logs([c], [a], bins, width)
            ref = T.numpy_timeline(pkg, [a], [sched], [c.accessTime], bins, width)
            assert host.same_as(ref), (c.nUE, bins, width, T.describe(host), T.describe(ref))


def test_invariants_against_the_oracles_results(pkg, trials):
    seen_restart = seen_truncated = False
    for c, res, a, sched in trials:
        bins = horizon(c, 1)
        t = pkg.timeline_from_logs([c], [a], bins, 1)
        s, sc = t.series, {f: int(v[0]) for f, v in t.scalars.items()}
        assert sc["arrival_overflow"] == 0 and sc["done_overflow"] == 0
        assert int(s["arrivals"].sum()) + sc["arrival_overflow"] == sc["arrived"] == res.activeCheck
        assert int(s["success"].sum()) == sc["success"] == int(s["done"].sum()) + sc["done_overflow"] == res.nSuccessUE
        assert int(s["timer_sum"].sum()) == sc["timer_sum"] == res.sumTimer
        assert int(s["sojourn_sum"].sum()) == sc["sojourn_sum"] >= sc["timer_sum"]
        assert (sc["sojourn_sum"] == sc["timer_sum"]) == (sc["restarted"] == 0)
        at, arrived, ok, done = T.per_ue(a, sched, c.accessTime)
        assert ((done - a[:, T.TIMER])[ok] >= at[ok]).all()      # the last cycle of a UE starts at its arrival or later
        assert (arrived == (at < res.steps)).all()               # arrived <=> its access slot was executed
        assert sc["done_max"] == (int(done[ok].max()) if ok.any() else -1)
        # the same invariants with both axes cut short of the horizon
        cut = pkg.timeline_from_logs([c], [a], 300, 5)
        k = {f: int(v[0]) for f, v in cut.scalars.items()}
        assert int(cut.series["arrivals"].sum()) + k["arrival_overflow"] == res.activeCheck and int(cut.series["done"].sum()) + k["done_overflow"] == res.nSuccessUE
        assert {f: k[f] for f in ("arrived", "success", "restarted", "sojourn_sum", "timer_sum", "done_max")} == {f: sc[f] for f in ("arrived", "success", "restarted", "sojourn_sum", "timer_sum", "done_max")}
        seen_restart |= sc["restarted"] > sc["success"] // 2 and sc["sojourn_sum"] > 10 * sc["timer_sum"]
        seen_truncated |= sc["arrived"] < c.nUE
    assert seen_restart and seen_truncated
    c, res, a, _ = trials[4]  # the overloaded trial: the reference's delay is the length of the last cycle only
    t = pkg.timeline_from_logs([c], [a], 10006, 1)
    assert (int(t.scalars["success"][0]), int(t.scalars["restarted"][0]), int(t.scalars["timer_sum"][0]), int(t.scalars["sojourn_sum"][0]),
            int(t.scalars["done_max"][0])) == (17782, 15381, 842947, 30210018, 10003)


def test_synthetic_edges_and_refusals(pkg):
    c = pkg.make_cfg(200, variant=0, rng_mode=pkg.RNG_PHILOX, seed=0)
    sched = pkg.arrival_schedule(c)[0]
    at = 5 * np.searchsorted(np.asarray(sched), np.arange(200), side="right")
    a = np.zeros((200, 16), dtype=np.int32)
    a[:, 0] = np.arange(200)
    a[:, T.ACTIVE] = np.where(np.arange(200) % 5 == 4, -1, 1)  # every fifth UE has not arrived, whatever the schedule says
    ok = np.arange(200) % 3 == 0
    a[ok, T.FLAG], a[ok, T.ACTIVE] = 1, 0
    a[ok, T.TXTIME] = at[ok] + np.arange(200)[ok] % 40        # completion = arrival + 6 .. + 45
    a[ok, T.TIMER] = np.where(np.arange(200)[ok] % 2 == 0, a[ok, T.TXTIME] + 6 - at[ok], 3)  # half of them never started over
    a[~ok, T.TIMER], a[~ok, T.TXTIME] = -7, -1                 # (an unfinished UE's timer and txTime are never read)
    for bins, width in ((1, 1), (7, 3), (4000, 1), (65536, 1)):
        host = pkg.timeline_from_logs([c, c], [a, a[:200]], bins, width, groups=[0, 0])
        assert host.same_as(T.numpy_timeline(pkg, [a, a], [sched, sched], [5, 5], bins, width, groups=[0, 0])), (bins, width)
    t = pkg.timeline_from_logs([c], [a], 4000, 1)
    assert int(t.scalars["arrived"][0]) == int((a[:, T.ACTIVE] != -1).sum()) and 0 < int(t.scalars["restarted"][0]) < int(t.scalars["success"][0])
    none = pkg.timeline_from_logs([c], [np.where(np.arange(16) == T.ACTIVE, -1, 0).astype(np.int32)[None, :].repeat(200, 0)], 16, 2)
    assert int(none.scalars["done_max"][0]) == -1 and int(none.scalars["arrived"][0]) == 0 and int(none.scalars["trials"][0]) == 1 and not any(v.any() for v in none.series.values())
    for col, val in ((T.TIMER, -3), (T.TXTIME, -100)):  # a successful UE with a negative timer / a completion before its arrival: refused, nothing added
        b = a.copy()
        b[150, col] = val
        assert b[150, T.FLAG] == 1
        with pytest.raises(pkg.PrachError) as ei:
            pkg.timeline_from_logs([c], [b], 16, 2)
        assert ei.value.status == -1
    for bins, width in ((0, 1), (65537, 1), (16, 0)):
        with pytest.raises(pkg.PrachError) as ei:
            pkg.timeline_from_logs([c], [a], bins, width)
        assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # the log is not this config's
        pkg.timeline_from_logs([c], [a[:199]], 16, 2)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c logs no trace of a cycle start
        pkg.timeline_from_logs([pkg.make_cfg(200, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX)], [a], 16, 2)
    assert ei.value.status == -2


def test_merge_of_two_halves_is_the_whole(pkg, trials):
    cfgs, logs = [t[0] for t in trials[:4]], [t[2] for t in trials[:4]]
    whole = pkg.timeline_from_logs(cfgs, logs, 700, 9, groups=[0, 0, 0, 0])
    left = pkg.timeline_from_logs(cfgs[:2], logs[:2], 700, 9, groups=[0, 0])
    right = pkg.timeline_from_logs(cfgs[2:], logs[2:], 700, 9, groups=[0, 0])
    assert int(left.scalars["done_max"][0]) != int(right.scalars["done_max"][0])
    left.merge_group(0, right, 0)
    assert left.same_as(whole) and int(whole.scalars["arrival_overflow"][0]) > 0 and int(whole.scalars["done_overflow"][0]) > 0
    empty = pkg.Timeline(1, 700, 9)
    empty.merge_group(0, pkg.Timeline(1, 700, 9), 0)
    assert int(empty.scalars["done_max"][0]) == -1 and int(empty.scalars["trials"][0]) == 0
    empty.merge_group(0, whole, 0)
    assert empty.same_as(whole)


def test_csv_is_pinned(pkg):
    c = pkg.make_cfg(6, variant=0, rng_mode=pkg.RNG_PHILOX, seed=0)
    assert pkg.arrival_schedule(c)[0][:2] == [0, 1]  # UE 0 arrives in slot 1 (5 ms); every slot from there on takes one more UE
    a = np.zeros((6, 16), dtype=np.int32)
    a[:, T.ACTIVE] = [0, 0, 1, 0, -1, -1]
    a[:, T.FLAG] = [1, 1, 0, 1, 0, 0]
    a[:, T.TXTIME] = [10, 30, 0, 200, 0, 0]  # completions 16, 36, -, 206
    a[:, T.TIMER] = [11, 4, 9, 186, 0, 0]    # UE 0 (arrival 5) and UE 3 (arrival 20) never started over, UE 1 (arrival 10) did
    t = pkg.timeline_from_logs([c], [a], 5, 10)  # bins [0,10) .. [40,50): the completion at 206 overflows
    assert pkg.timeline_csv(t, labels=["6"]) == (b"6,arrivals,0,1\n6,arrivals,10,2\n6,arrivals,20,1\n6,success,0,1\n6,success,10,1\n6,success,20,1\n"
                                                 b"6,sojourn_sum,0,11\n6,sojourn_sum,10,26\n6,sojourn_sum,20,186\n6,timer_sum,0,11\n6,timer_sum,10,4\n6,timer_sum,20,186\n"
                                                 b"6,done,10,1\n6,done,30,1\n6,done,overflow,1\n")
    assert [int(t.scalars[f][0]) for f in ("arrived", "success", "restarted", "done_overflow", "done_max")] == [4, 3, 1, 1, 206]
    cut = pkg.timeline_from_logs([c], [a], 2, 5)  # bins [0,5) [5,10): the arrivals at 10, 15 and 20 overflow
    assert pkg.timeline_csv(cut) == b"0,arrivals,5,1\n0,arrivals,overflow,3\n0,success,5,1\n0,sojourn_sum,5,11\n0,timer_sum,5,11\n0,done,overflow,3\n"
    sp, g, ser = t.spec(), t._group(0), t._series(0)
    need = pkg.lib().prach_timeline_format_csv(C.byref(sp), C.byref(g), ser, b"6", None, 0)
    small = C.create_string_buffer(b"x" * 40, 41)
    assert pkg.lib().prach_timeline_format_csv(C.byref(sp), C.byref(g), ser, b"6", small, 40) == need and small.value == b""  # does not fit: the length only
    assert pkg.timeline_csv(pkg.Timeline(2, 5, 10)) == b""


def test_run_trials_timeline_argument_errors_need_no_device(pkg):
    """Spec, groups and variants are judged before the engine is looked at: without any engine a NOMA.c trial or a request that is too large is
    PRACH_ERR_UNSUPPORTED, not PRACH_ERR_ARG."""
    L = pkg.lib()
    n = 3
    res = (pkg.PrachResult * n)()
    tt = (pkg.PrachTimeline * 8)()
    ser = [(C.c_uint64 * (8 * 16))() for _ in range(5)]

    def call(bins=16, width=1, ngroups=3, reserved=0, group=None, tl=tt, series=ser, spec=True, nn=n, variants=(0, 1, 0)):
        cfgs = (pkg.PrachCfg * n)(*[pkg.make_cfg(100, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s, v in enumerate(variants)])
        sp = pkg.PrachTimelineSpec(bins, width, ngroups, reserved)
        gp = None if group is None else (C.c_int32 * len(group))(*group)
        return L.prach_run_trials_timeline(None, cfgs, nn, res, None, C.byref(sp) if spec else None, gp, tl, *series)

    assert call() == -1  # everything in order but the engine
    assert call(variants=(0, 2, 1)) == -2  # a NOMA.c trial: refused before anything could be launched
    assert call(ngroups=500, bins=65536, group=[0, 1, 2]) == -2  # 5 x 500 x 65536 words > 2^27
    assert call(ngroups=400, bins=65536, group=[0, 399, 5]) == -1  # 5 x 400 x 65536 words <= 2^27: accepted as far as the missing engine
    bad_series = [ser[:q] + [None] + ser[q + 1:] for q in range(5)]
    for bad in [dict(bins=0), dict(bins=65537), dict(width=0), dict(ngroups=0), dict(ngroups=4), dict(reserved=1), dict(group=[0, 1, 3]), dict(group=[0, -1, 2]),
                dict(tl=None), dict(spec=False), dict(nn=0)] + [dict(series=b) for b in bad_series]:
        assert call(**bad) == -1, bad
    assert call(ngroups=500, bins=65536, group=[0, 500, 1]) == -1  # a bad group id in a request that is also too large is an argument error
    assert call(variants=(2, 2, 2), group=[0, 1, 7]) == -1         # ... and in one with a NOMA.c trial
    tile, window = pkg.timeline_tile_ues(), pkg.timeline_window_bins()
    assert tile >= 1024 and tile % 64 == 0 and tile * (60000 + 6) < 2 ** 32 and 64 <= window <= pkg.TIMELINE_MAX_BINS


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_trial(pkg, rank):
    """A synthetic trial per rank: every UE arrived, two thirds succeeded (none on rank 1's second trial)."""
    out = []
    for k, n in enumerate((300 + 40 * rank, 77)):
        c = pkg.make_cfg(n, variant=rank, rng_mode=pkg.RNG_PHILOX, seed=rank)
        at = 5 * np.searchsorted(np.asarray(pkg.arrival_schedule(c)[0]), np.arange(n), side="right")
        rng = np.random.default_rng(10 * rank + k)
        a = np.zeros((n, 16), dtype=np.int32)
        ok = (np.arange(n) % 3 != 0) & (not (rank == 1 and k == 1))
        a[ok, T.FLAG] = 1
        a[:, T.TXTIME] = at + rng.integers(0, 200 + 100 * rank, n)
        a[:, T.TIMER] = rng.integers(0, a[:, T.TXTIME] + 7 - at)
        out.append((c, a))
    return out


def _allreduce_worker(rank, world, port, q):
    import importlib
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    distmod = importlib.import_module("nr_randomaccess_amd.dist")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = _rank_trial(pkg, rank)
    t = pkg.timeline_from_logs([c for c, _ in mine], [a for _, a in mine], 64, 40, groups=[0, 2], ngroups=3)  # (group 1 stays empty on every rank)
    distmod.allreduce_timeline(t)
    q.put((rank, {n: t.series[n].tolist() for n in pkg.TIMELINE_SERIES}, {f: t.scalars[f].tolist() for f in pkg.TIMELINE_FIELDS}))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_timeline_two_ranks_gloo(pkg):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_allreduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    tr = [_rank_trial(pkg, r) for r in range(world)]
    order = [tr[0][0], tr[1][0], tr[0][1], tr[1][1]]
    exp = pkg.timeline_from_logs([c for c, _ in order], [a for _, a in order], 64, 40, groups=[0, 0, 2, 2], ngroups=3)
    for _, series, scalars in outs:  # every rank holds the merged block
        assert series == {n: exp.series[n].tolist() for n in pkg.TIMELINE_SERIES}
        assert scalars == {f: exp.scalars[f].tolist() for f in pkg.TIMELINE_FIELDS}
    assert exp.scalars["done_max"].tolist()[1] == -1 and exp.scalars["trials"].tolist() == [2, 0, 2] and int(exp.scalars["success"][2]) > 0
    assert int(exp.scalars["done_max"][0]) > 0 and int(exp.scalars["done_overflow"].sum()) >= 0
