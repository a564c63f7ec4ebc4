"""Host side of the per-trial distributions (include/prach.h, prach_dist_*): the definition prach::dist_kernel must equal, the merge, the
quantile, the CSV text, the all-reduce of dist.py and the argument checks of prach_run_trials_dist that need no device.  No GPU."""
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

TIMER, PTC, FLAG = 1, 11, 14  # columns of the 16-field per-UE log


def synth_logs(n, seed, max_timer, flags=(0, 1), ptcs=(0, 1, 2, 3, 254, 255, 300)):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 16), dtype=np.int32)
    a[:, 0] = np.arange(n)
    a[:, TIMER] = rng.integers(0, max_timer + 1, n)
    a[:, PTC] = rng.choice(ptcs, n)
    a[:, FLAG] = rng.choice(flags, n)
    a[a[:, FLAG] == 0, TIMER] = rng.integers(-5, 50, int((a[:, FLAG] == 0).sum()))  # (an unfinished UE's timer is never read)
    return a


def expect(logs_list, bins, width):
    """np.bincount form of one group over the given trials' logs."""
    t = np.concatenate([a[a[:, FLAG] == 1, TIMER] for a in logs_list]).astype(np.int64)
    p = np.concatenate([a[a[:, FLAG] == 1, PTC] for a in logs_list]).astype(np.int64)
    b = t // width
    return dict(delay_hist=np.bincount(b[b < bins], minlength=bins).astype(np.uint64),
                ptc_hist=np.bincount(np.minimum(p, 255), minlength=256).astype(np.uint64),
                trials=len(logs_list), ues=sum(len(a) for a in logs_list), success=t.size, delay_overflow=int((b >= bins).sum()),
                delay_sum=int(t.sum()), ptc_sum=int(p.sum()), delay_max=int(t.max()) if t.size else -1)


def assert_group(d, g, e):
    assert np.array_equal(d.delay_hist[g], e["delay_hist"])
    assert np.array_equal(d.ptc_hist[g], e["ptc_hist"])
    for f in ("trials", "ues", "success", "delay_overflow", "delay_sum", "ptc_sum", "delay_max"):
        assert int(getattr(d, f)[g]) == e[f], (f, int(getattr(d, f)[g]), e[f])


@pytest.mark.parametrize("bins", [1, 7, 16384])
@pytest.mark.parametrize("width", [1, 3, 5])
def test_accumulate_logs_equals_bincount(pkg, bins, width):
    edge = bins * width
    a = synth_logs(5000, 7 * bins + width, min(edge + 2 * width, 70000))
    # timers exactly on bin edges and on either side of the overflow edge; every preamble count of interest among the successful UEs
    for k, (t, p) in enumerate([(0, 0), (width, 254), (width - 1 if width > 1 else 0, 255), (edge - 1, 300), (edge, 1), (edge + 1, 2), ((bins - 1) * width, 3)]):
        a[k, TIMER], a[k, PTC], a[k, FLAG] = t, p, 1
    b = synth_logs(37, 99, edge)
    d = pkg.dist_from_logs([a, b], bins, width, groups=[0, 0])
    assert_group(d, 0, expect([a, b], bins, width))
    assert int(d.delay_overflow[0]) >= 2


def test_accumulate_logs_no_successful_ue_and_bad_input(pkg):
    a = synth_logs(300, 1, 100, flags=(0,))
    d = pkg.dist_from_logs([a], 16, 2)
    assert_group(d, 0, expect([a], 16, 2))
    assert int(d.delay_max[0]) == -1 and int(d.success[0]) == 0 and int(d.trials[0]) == 1 and not d.delay_hist.any() and not d.ptc_hist.any()
    a[5, FLAG], a[5, TIMER] = 1, -3  # a successful UE cannot have a negative delay: refused, nothing added
    with pytest.raises(pkg.PrachError) as ei:
        pkg.dist_from_logs([a], 16, 2)
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError):
        pkg.dist_from_logs([a], 0, 1)
    with pytest.raises(pkg.PrachError):
        pkg.dist_from_logs([a], 16385, 1)
    with pytest.raises(pkg.PrachError):
        pkg.dist_from_logs([a], 16, 0)


@pytest.fixture(scope="module")
def oracle_trials(ob):
    """(log as int32 [nUE, 16], sumTimer, preambleTxCount) of a Beta.c and a RandomAccessWithNOMA trial (12 grants) and of a NOMA.c trial."""
    out = []
    for variant, n, seed in ((0, 3000, 1), (1, 20000, 2)):
        res, ues = ob.run_trial(ob.make_cfg(n, variant=variant, nGrantUL=12), ob.Rng(ob.RNG_PHILOX, seed))
        out.append((np.frombuffer(ues, dtype=np.int32).reshape(-1, 16).copy(), res.sumTimer, res.preambleTxCount))
    res, ues = ob.noma_run_trial(ob.make_noma_cfg(3000, nGrantUL=12), ob.Rng(ob.RNG_PHILOX, 3))
    noma_ue = np.dtype([("i", np.int32, 16), ("g", np.float64)])
    out.append((np.frombuffer(ues, dtype=noma_ue)["i"].copy(), res.delay, res.nTxP))  # (RA sits in the msg4Flag column, nTxPreamble in preambleTxCounter's)
    return out


@pytest.mark.parametrize("bins,width", [(4096, 1), (64, 7)])
def test_accumulate_oracle_trials(pkg, oracle_trials, bins, width):
    d = pkg.dist_from_logs([a for a, _, _ in oracle_trials], bins, width)
    for g, (a, sum_timer, ptc_count) in enumerate(oracle_trials):
        assert_group(d, g, expect([a], bins, width))
        assert int(d.success[g]) > 0
        assert int(d.delay_sum[g]) == sum_timer and int(d.ptc_sum[g]) == ptc_count


def test_quantile_is_the_sorted_definition(pkg, oracle_trials):
    a = oracle_trials[0][0]
    delays = np.sort(a[a[:, FLAG] == 1, TIMER])
    d = pkg.dist_from_logs([a], 16384, 1)
    assert int(d.delay_overflow[0]) == 0
    for q in (0.1, 0.5, 0.9, 1.0):
        assert pkg.dist_quantile(d, 0, q) == int(delays[math.ceil(q * delays.size) - 1]), q
    assert pkg.dist_quantile(d, 0, 0.0) == int(delays[0])  # (rank at least 1)
    w = pkg.dist_from_logs([a], 4096, 5)
    assert pkg.dist_quantile(w, 0, 0.5) == int(delays[math.ceil(0.5 * delays.size) - 1]) // 5 * 5  # lower edge of the bin
    # -1: no successful UE; the rank falls into the overflow
    assert pkg.dist_quantile(pkg.dist_from_logs([synth_logs(10, 1, 5, flags=(0,))], 8, 1), 0, 0.5) == -1
    assert delays[-1] > delays[math.ceil(0.1 * delays.size) - 1]
    cut = pkg.dist_from_logs([a], int(delays[-1]), 1)  # the largest delays fall off the last bin
    assert int(cut.delay_overflow[0]) > 0 and pkg.dist_quantile(cut, 0, 1.0) == -1 and pkg.dist_quantile(cut, 0, 0.1) == int(delays[math.ceil(0.1 * delays.size) - 1])


def test_csv_is_pinned(pkg):
    a = np.zeros((5, 16), dtype=np.int32)
    a[:, TIMER] = [12, 3, 12, 40, 7]
    a[:, PTC] = [1, 2, 1, 300, 1]
    a[:, FLAG] = [1, 1, 1, 1, 0]
    d = pkg.dist_from_logs([a], 4, 5)  # bins [0,5) [5,10) [10,15) [15,20); 40 overflows; UE 4 did not succeed
    assert pkg.dist_csv(d, labels=["10000"]) == (b"10000,delay,0,1,0.250000\n10000,delay,10,2,0.750000\n10000,delay,overflow,1,1.000000\n"
                                                 b"10000,ptx,1,2,0.500000\n10000,ptx,2,1,0.750000\n10000,ptx,255,1,1.000000\n")
    sp, g = d.spec(), d._group(0)
    dh, ph = d._hists(0)
    need = pkg.lib().prach_dist_format_csv(C.byref(sp), C.byref(g), dh, ph, b"10000", None, 0)
    small = C.create_string_buffer(b"x" * 40, 41)
    assert pkg.lib().prach_dist_format_csv(C.byref(sp), C.byref(g), dh, ph, b"10000", small, 40) == need and small.value == b""  # does not fit: the length only
    assert pkg.dist_csv(pkg.dist_from_logs([a[4:]], 4, 5)) == b""  # no successful UE: no line


def test_merge_of_two_halves_is_the_whole(pkg, oracle_trials):
    logs = [a for a, _, _ in oracle_trials] + [synth_logs(100, 5, 10, flags=(0,))]
    whole = pkg.dist_from_logs(logs, 512, 3, groups=[0, 0, 0, 0])
    left = pkg.dist_from_logs(logs[:2], 512, 3, groups=[0, 0])
    right = pkg.dist_from_logs(logs[2:], 512, 3, groups=[0, 0])
    left.merge_group(0, right, 0)
    assert left.same_as(whole)
    empty = pkg.Dist(1, 512, 3)
    empty.merge_group(0, pkg.Dist(1, 512, 3), 0)
    assert int(empty.delay_max[0]) == -1 and int(empty.trials[0]) == 0
    empty.merge_group(0, whole, 0)
    assert empty.same_as(whole)


def test_run_trials_dist_argument_errors_need_no_device(pkg):
    """The spec is judged before the engine is looked at: without any engine a request that is too large is PRACH_ERR_UNSUPPORTED, not PRACH_ERR_ARG."""
    L = pkg.lib()
    n = 3
    cfgs = (pkg.PrachCfg * n)(*[pkg.make_cfg(100, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(n)])
    res = (pkg.PrachResult * n)()
    dd = (pkg.PrachDist * 8)()
    dh, ph = (C.c_uint64 * (8 * 16))(), (C.c_uint64 * (8 * 256))()

    def call(bins=16, width=1, ngroups=3, reserved=0, group=None, dist=dd, delay=dh, ptc=ph, spec=True, nn=n):
        sp = pkg.PrachDistSpec(bins, width, ngroups, reserved)
        gp = None if group is None else (C.c_int32 * len(group))(*group)
        return L.prach_run_trials_dist(None, cfgs, nn, res, None, C.byref(sp) if spec else None, gp, dist, delay, ptc)

    assert call() == -1  # everything in order but the engine
    assert call(ngroups=8100, bins=16384, group=[0, 1, 2]) == -2  # 8100 x (16384 + 256) words > 2^27
    assert call(ngroups=8000, bins=16384, group=[0, 7999, 5]) == -1  # 8000 x 16640 words <= 2^27: accepted as far as the missing engine
    for bad in (dict(bins=0), dict(bins=16385), dict(width=0), dict(ngroups=0), dict(ngroups=4), dict(reserved=1), dict(group=[0, 1, 3]), dict(group=[0, -1, 2]),
                dict(dist=None), dict(delay=None), dict(ptc=None), dict(spec=False), dict(nn=0)):
        assert call(**bad) == -1, bad
    # the checks come before the size limit is looked at: a bad group id in a request that is also too large is an argument error
    assert call(ngroups=8100, bins=16384, group=[0, 8100, 1]) == -1
    assert pkg.dist_tile_ues() >= 1024 and pkg.dist_tile_ues() % 1024 == 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_logs(rank):
    return [synth_logs(400 + 50 * rank, 10 + rank, 300), synth_logs(77, 20 + rank, 300, flags=(0,) if rank else (0, 1))]


def _allreduce_worker(rank, world, port, q):
    import importlib
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    distmod = importlib.import_module("nr_randomaccess_amd.dist")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = pkg.dist_from_logs(_rank_logs(rank), 64, 4, groups=[0, 2], ngroups=3)  # (group 1 stays empty on every rank)
    distmod.allreduce_dist(d)
    q.put((rank, d.delay_hist.tolist(), d.ptc_hist.tolist(), {f: getattr(d, f).tolist() for f in pkg.DIST_FIELDS}))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_dist_two_ranks_gloo(pkg):
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
    logs = [_rank_logs(r) for r in range(world)]
    exp = pkg.dist_from_logs([logs[0][0], logs[1][0], logs[0][1], logs[1][1]], 64, 4, groups=[0, 0, 2, 2], ngroups=3)
    for _, dh, ph, fields in outs:  # every rank holds the merged block
        assert dh == exp.delay_hist.tolist() and ph == exp.ptc_hist.tolist()
        assert fields == {f: getattr(exp, f).tolist() for f in pkg.DIST_FIELDS}
    assert exp.delay_max.tolist()[1] == -1 and exp.trials.tolist() == [2, 0, 2]
