"""The per-subframe preamble trace without a GPU: the oracle reference against itself (tests/tools/trace_ref.py), the host side of the C ABI
(prach_trace_merge, prach_trace_format_csv, struct sizes, argument errors that need no device), the CLI's refusal, the binding's Trace and
dist.allreduce_trace under gloo.  (sweep.py --trace needs a device: tests/test_gpu_trace_sweep.py.)"""
import ctypes as C
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import trace_cases as TC  # noqa: E402
import trace_ref as TR  # noqa: E402


def _cases():
    out = []
    for k, (name, n, kw) in enumerate(TC.CASES):
        out += [(v, n, kw, k % 2, 100 * k + v) for v in (0, 1)]
    name, n, kw = TC.SECTOR
    return out + [(1, n, kw, 0, 41), (1, n, kw, 1, 41)]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"v{c[0]}_n{c[1]}_rng{c[3]}")
def test_reference_against_itself(ob, case):
    """The census and the prefix runs are two views of one oracle: at every edge txop - collisions of the prefix run is the census's cumulative singles, and
    for Beta.c txop is the cumulative calls.  At most 16 edges, spread evenly, the last step included."""
    r = TR.ref(case)
    assert 1 <= len(r.edges) <= 16 and r.edges[-1] == r.steps == int(r.res.steps)
    assert r.check_self() == 0
    assert (r.singles <= r.calls).all() and (r.singles >= 0).all()  # (a preamble can be called on more than once per subframe: calls may exceed nPreamble)
    if case[1] == 3000 and not case[2].get("sector_grants"):
        assert r.calls.max() > 50 and all((r.calls[np.arange(r.steps) % 5 == m] > 0).any() for m in range(5))  # over_3000: all five residues of t % 5 occur


def test_reference_every_subframe_and_uniform(ob):
    name, n, kw = TC.EVERY
    r = TR.ref((1, n, kw, 1, 43), every=True)
    assert r.steps == 1500 == len(r.prefix) and r.check_self() == 0
    # consecutive edges pin every single subframe of the two weighted series
    st = r.stretches()
    assert [hi - lo for lo, hi, _, _ in st] == [1] * 1500
    x, q = np.array([s[2] for s in st]), np.array([s[3] for s in st])
    assert np.array_equal(x - q, r.singles) and ((x == 0) == (r.calls == 0)).all()
    storm = (0, 2600, dict(uniform=1, nPreamble=54, backoff=5, nGrantUL=1, maxRarWindow=1, maxMsg2TxCount=0, accessTime=10), 1, 600)
    u = TR.ref(storm, 6)
    assert u.steps == 60000 and len(u.edges) <= 6 and u.check_self() == 0


def _filled(pkg, seed, ngroups=2, bins=8, bin_ms=5):
    rng = np.random.default_rng(seed)
    t = pkg.Trace(ngroups, bins, bin_ms)
    for n in pkg.TRACE_SERIES:
        t.series[n][:] = rng.integers(0, 2 ** 40, (ngroups, bins), dtype=np.uint64)
    for f in pkg.TRACE_FIELDS:
        t.scalars[f][:] = rng.integers(0, 2 ** 40, ngroups)
    return t


def test_merge(pkg):
    a, b, c = _filled(pkg, 1), _filled(pkg, 2), _filled(pkg, 3)
    b.scalars["subframes"][1] = 0  # an empty group's calls_max does not count, whatever it holds
    b.scalars["calls_max"][1] = 2 ** 50
    exp_series = {n: a.series[n] + b.series[n] + c.series[n] for n in pkg.TRACE_SERIES}
    exp_sc = {f: a.scalars[f] + b.scalars[f] + c.scalars[f] for f in pkg.TRACE_FIELDS if f != "calls_max"}
    exp_max = [max(int(a.scalars["calls_max"][0]), int(b.scalars["calls_max"][0]), int(c.scalars["calls_max"][0])),
               max(int(a.scalars["calls_max"][1]), int(c.scalars["calls_max"][1]))]
    left = _filled(pkg, 1).merge(b).merge(c)
    bc = _filled(pkg, 2)
    bc.scalars["subframes"][1] = 0
    bc.scalars["calls_max"][1] = 2 ** 50
    right = _filled(pkg, 1).merge(bc.merge(c))
    for m in (left, right):
        for n in pkg.TRACE_SERIES:
            assert np.array_equal(m.series[n], exp_series[n])
        for f, v in exp_sc.items():
            assert np.array_equal(m.scalars[f], v), f
        assert m.scalars["calls_max"].tolist() == exp_max
    assert left.same_as(right)
    empty = pkg.Trace(2, 8, 5)
    assert empty.merge(pkg.Trace(2, 8, 5)).scalars["calls_max"].tolist() == [-1, -1]
    with pytest.raises(ValueError):
        empty.merge(pkg.Trace(2, 9, 5))
    # NULL arguments and a bad spec leave `into` alone
    L = pkg.lib()
    sp, ta, tb = pkg.PrachTraceSpec(0, 5, 1, 0), pkg.PrachTrace(), pkg.PrachTrace(trials=3)
    L.prach_trace_merge(C.byref(sp), C.byref(ta), a._series(0), C.byref(tb), b._series(0))
    assert ta.trials == 0


def test_format_csv_on_a_hand_written_group(pkg):
    t = pkg.Trace(1, 4, 7)
    t.series["calls"][0] = [3, 0, 5, 0]
    t.series["singles"][0] = [1, 0, 0, 0]
    t.series["txop"][0] = [3, 0, 12, 0]
    t.series["collisions"][0] = [2, 0, 12, 0]
    t.scalars["overflow_calls"][0] = 9
    assert t.csv(labels=["3000"]) == (b"3000,calls,0,3\n3000,calls,14,5\n3000,singles,0,1\n3000,txop,0,3\n3000,txop,14,12\n3000,collisions,0,2\n3000,collisions,14,12\n"
                                      b"3000,calls,overflow,9\n")
    assert pkg.trace_csv(t, labels=["3000"]) == t.csv(labels=["3000"])
    t.scalars["overflow_calls"][0] = 0
    assert t.csv().endswith(b"0,collisions,14,12\n")
    ratio = t.collision_ratio(0)
    assert ratio[0] == pytest.approx(2 / 3) and ratio[2] == 1.0 and np.isnan(ratio[1]) and np.isnan(ratio[3])
    # the size is returned without a buffer, and a buffer that is too small gets no partial text
    L = pkg.lib()
    sp, d = t.spec(), t._group(0)
    need = L.prach_trace_format_csv(C.byref(sp), C.byref(d), t._series(0), b"3000", None, 0)
    buf = C.create_string_buffer(b"x" * 10, 10)
    assert L.prach_trace_format_csv(C.byref(sp), C.byref(d), t._series(0), b"3000", buf, 10) == need and buf.raw[0] == 0


def test_struct_sizes_match_a_compiled_check(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "prach.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(prach_trace_spec), sizeof(prach_trace),'
                   ' sizeof(prach_timing), offsetof(prach_timing, trace_ms), offsetof(prach_trace, calls_max), PRACH_TRACE_MAX_BINS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert sizes == [C.sizeof(pkg.PrachTraceSpec), C.sizeof(pkg.PrachTrace), C.sizeof(pkg.PrachTiming), pkg.PrachTiming.trace_ms.offset, pkg.PrachTrace.calls_max.offset,
                     pkg.TRACE_MAX_BINS]
    assert sizes[:2] == [16, 64]
    for sym in ("prach_run_trials_trace", "prach_trace_merge", "prach_trace_format_csv", "prach_trace_tile_subframes"):
        assert sym in pkg.EXPORTS
    tile = pkg.trace_tile_subframes()
    assert tile >= 1024 and tile % 256 == 0


def test_run_trials_trace_argument_errors_need_no_device(pkg):
    """Spec, groups and variants are judged before the engine is looked at: word for word the rules of prach_run_trials_timeline."""
    L = pkg.lib()
    n = 3
    res = (pkg.PrachResult * n)()
    tt = (pkg.PrachTrace * 8)()
    arrs = [(C.c_uint64 * 16)() for _ in range(4)]

    def call(bins=2, bin_ms=1, ngroups=3, reserved=0, group=None, tr=tt, arrays=arrs, spec=True, nn=n, variants=(0, 1, 0)):
        cfgs = (pkg.PrachCfg * n)(*[pkg.make_cfg(100, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s, v in enumerate(variants)])
        sp = pkg.PrachTraceSpec(bins, bin_ms, ngroups, reserved)
        gp = None if group is None else (C.c_int32 * len(group))(*group)
        return L.prach_run_trials_trace(None, cfgs, nn, res, None, C.byref(sp) if spec else None, gp, tr, *arrays)

    assert call() == -1  # everything in order but the engine
    assert call(variants=(0, 2, 1)) == -2  # a NOMA.c trial: refused before anything could be launched
    assert call(ngroups=600, bins=65536, group=[0, 599, 1]) == -2  # 4 x 600 x 65536 words > 2^27
    assert call(ngroups=512, bins=65536, group=[0, 511, 1]) == -1  # exactly 2^27: accepted as far as the missing engine
    bad_arrays = [arrs[:q] + [None] + arrs[q + 1:] for q in range(4)]
    for bad in [dict(bins=0), dict(bins=65537), dict(bin_ms=0), dict(ngroups=0), dict(ngroups=4), dict(reserved=1), dict(group=[0, 1, 3]), dict(group=[0, -1, 2]),
                dict(tr=None), dict(spec=False), dict(nn=0)] + [dict(arrays=b) for b in bad_arrays]:
        assert call(**bad) == -1, bad
    assert call(variants=(2, 2, 2), group=[0, 1, 7]) == -1  # a bad group id in a call with a NOMA.c trial is an argument error


def test_cli_refuses_trace_with_another_reduction(pkg, tmp_path):
    for other in (["--cdf", "c.csv"], ["--timeline", "t.csv"], ["--sojourn", "s.csv"], ["--ci", "i.csv"]):
        p = subprocess.run([pkg.CLI_PATH, "--trace", str(tmp_path / "x.csv")] + other, capture_output=True, text=True)
        assert p.returncode == 255 and "--trace cannot be combined" in p.stdout and "one reduction per call" in p.stdout
    p = subprocess.run([pkg.CLI_PATH, "--program", "noma", "--trace", str(tmp_path / "x.csv")], capture_output=True, text=True)
    assert p.returncode == 255 and "--trace needs --program beta or withnoma" in p.stdout
    p = subprocess.run([pkg.CLI_PATH, "--trace", str(tmp_path / "x.csv"), "--trace-bin", "0"], capture_output=True, text=True)
    assert p.returncode == 255 and not (tmp_path / "x.csv").exists()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_trace(pkg, rank):
    t = _filled(pkg, 50 + rank, ngroups=3, bins=12, bin_ms=7)
    for n in pkg.TRACE_SERIES:  # group 1 stays empty on every rank
        t.series[n][1] = 0
    for f in pkg.TRACE_FIELDS:
        t.scalars[f][1] = -1 if f == "calls_max" else 0
    return t


def _allreduce_worker(rank, world, port, q):
    import importlib
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    distmod = importlib.import_module("nr_randomaccess_amd.dist")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = _rank_trace(pkg, rank)
    distmod.allreduce_trace(t)
    q.put((rank, [x.tolist() for x in t._arrays()], {f: t.scalars[f].tolist() for f in pkg.TRACE_FIELDS}))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_trace_two_ranks_gloo(pkg):
    """One int64 sum all-reduce, calls_max by max: every rank ends with what prach_trace_merge makes of the two."""
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
    exp = _rank_trace(pkg, 0).merge(_rank_trace(pkg, 1))
    for _, arrays, scalars in outs:
        assert arrays == [x.tolist() for x in exp._arrays()]
        assert scalars == {f: exp.scalars[f].tolist() for f in pkg.TRACE_FIELDS}
    assert exp.scalars["calls_max"].tolist()[1] == -1 and exp.scalars["trials"].tolist()[1] == 0
