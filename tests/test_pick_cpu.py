"""Host side of the pick (include/prach.h, prach_pick_*): the definition prach::pick_kernel and the engine's sort must equal, against a numpy restatement
(the predicate on xtab_ref.values, np.lexsort on key and index) over the oracle's UEs and against the xtab and summary definitions already here; the CSV
text, the struct sizes, the gather of dist.py and the argument checks of prach_run_trials_pick that need no device.  No GPU."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import pick_ref as P  # noqa: E402
import timeline_ref as T  # noqa: E402
import xtab_ref as X  # noqa: E402
from test_xtab_cpu import CASES as XTAB_CASES, FIRST_CENSUS, OVERLOADED as XTAB_OVERLOADED  # noqa: E402

ALL = X.SERVED | X.UNSERVED | X.IDLE
# 37 UEs in the reference's stream; 4097 UEs; the overloaded 20 000-UE trial (UEs start over, 2218 unserved); a trial cut at subframe 2500 and the census
# trial cut at 4000 (idle UEs: undefined values)
CASES = [XTAB_CASES[k] for k in (2, 5, XTAB_OVERLOADED, 10, FIRST_CENSUS + 1)]
OVERLOADED, CUT = 2, 4
# (where, order, key, k, who): every field as key and as clause, every order, k of 1 and of the largest, clauses that nobody passes, undefined values
SPECS = [((), "index", None, 16, ALL), ((), "index", None, 1, X.UNSERVED), ((("state", 2, 3),), "index", None, 4096, X.UNSERVED | X.IDLE),
         ((), "largest", "sojourn", 16, X.SERVED), ((), "smallest", "sojourn", 16, X.SERVED), ((), "largest", "failcount", 16, ALL), ((), "largest", "ptc", 8, X.UNSERVED),
         ((("age", 0, 100000), ("timer", 5, 40)), "smallest", "timer", 7, X.UNSERVED | X.IDLE), ((("arrival", 2000, 2999), ("completion", 0, 5000)), "largest", "age", 100, ALL),
         ((("sojourn", 100, 65535), ("ptc", 2, 9), ("failcount", 0, 0), ("one", 0, 0)), "smallest", "completion", 33, ALL), ((), "largest", "one", 5, X.IDLE | X.SERVED),
         ((), "smallest", "state", 4096, ALL), ((("timer", 70000, 80000),), "largest", "timer", 3, ALL), ((("state", 0, 0),), "smallest", "arrival", 9, ALL),
         ((), "largest", "arrival", 1, ALL)]


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


def host_of(pkg, c, res, a, spec):
    return pkg.pick_from_logs([c], [res.steps], [a], *spec)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "{}-{}-{}-k{}-w{}".format("+".join(f for f, _, _ in s[0]) or "all", s[1], s[2], s[3], s[4]))
def test_from_logs_equals_numpy_on_oracle_ues(pkg, trials, spec):
    for c, res, a, sched in trials:
        pk = host_of(pkg, c, res, a, spec)
        P.check(pk, [P.numpy_pick(a, sched, c.accessTime, min(res.steps, res.maxTime), pk.where, pk.order, pk.key, pk.k, pk.who)])
        h = {f: int(pk.headers[f][0]) for f in P.HEADER}
        assert h["stored"] == min(h["matched"], pk.k) and h["matched"] + h["undefined"] <= h["selected"] <= c.nUE == h["nUE"]


def test_what_the_specs_reach(pkg, trials):
    """The cases are not vacuous: ties are cut, values are undefined, a predicate matches nobody, and k exceeds the matches."""
    c, res, a, _ = trials[OVERLOADED]
    pk = host_of(pkg, c, res, a, SPECS[6])  # LARGEST ptc over the unserved, k = 8
    assert int(pk.headers["ties_left_out"][0]) > 0 and int(pk.headers["matched"][0]) == 2218 and int(pk.headers["threshold"][0]) == int(pk.rows["key"][0, 7])
    pk = host_of(pkg, c, res, a, SPECS[12])  # nobody's timer is that long
    assert int(pk.headers["matched"][0]) == 0 and int(pk.headers["threshold"][0]) == -1 and not pk.rows["idx"].any()
    c, res, a, _ = trials[CUT]
    pk = host_of(pkg, c, res, a, SPECS[7])  # the idle UEs have neither an age nor a timer
    assert int(pk.headers["undefined"][0]) == c.nUE - res.activeCheck > 0
    pk = host_of(pkg, c, res, a, SPECS[13])  # ... and no arrival: the idle UEs are selected by their STATE and undefined by their key
    assert int(pk.headers["undefined"][0]) == c.nUE - res.activeCheck and int(pk.headers["matched"][0]) == 0
    pk = host_of(pkg, c, res, a, ((("state", 0, 0),), "index", None, 3, ALL))  # the same UEs by index: their arrival is -1
    assert pk.rows["arrival"][0].tolist() == [-1] * 3 and (pk.rows["active"][0] == -1).all()
    c, res, a, _ = trials[0]
    pk = host_of(pkg, c, res, a, SPECS[11])
    assert int(pk.headers["stored"][0]) == c.nUE < pk.k and pk.rows["idx"][0, :c.nUE].tolist() == sorted(range(c.nUE), key=lambda i: (X.states(a)[i], i))


def test_cell_clauses_select_exactly_the_cell(pkg, trials):
    """For every cell of the default census — the overflow bins included — the number of matches under Xtab.cell_clauses is that cell of xtab_from_logs."""
    for c, res, a, _ in trials:
        xt = pkg.xtab_from_logs([c], [res.steps], [a])
        total = 0
        for r in range(xt.cells.shape[1]):
            for q in range(xt.cells.shape[2]):
                pk = host_of(pkg, c, res, a, (xt.cell_clauses(r, q), "index", None, 1, xt.who))
                assert int(pk.headers["matched"][0]) == int(xt.cells[0, r, q]), (c.nUE, r, q)
                total += int(pk.headers["matched"][0])
        assert total == int(xt.scalars["binned"][0]) > 0
    xt = pkg.Xtab(1, ("arrival", 500, 20), ("state", 1, 7))
    assert xt.cell_clauses(3, 7) == [(1, 1500, 1999), (8, 7, 2 ** 31 - 1)] and xt.cell_clauses(20, 0) == [(1, 10000, 2 ** 31 - 1), (8, 0, 0)]
    with pytest.raises(ValueError):
        xt.cell_clauses(21, 0)


def test_cross_checks_against_the_summary(pkg, trials):
    """Row 0's key under LARGEST sojourn over the served is the summary's sojourn_max; the threshold at k = n - r + 1 is the summary's level of rank r (the
    k-th largest of n is the (n - k + 1)-th smallest), and under SMALLEST at k = r."""
    levels = (800, 950, 990, 1000)
    for c, res, a, _ in trials:
        sm = pkg.summary_from_logs([c], [a], levels).rows[0]
        n = int(sm["success"])
        if n == 0:
            continue
        top = host_of(pkg, c, res, a, ((), "largest", "sojourn", 16, X.SERVED))
        assert int(top.rows["key"][0, 0]) == int(sm["sojourn_max"]) and int(top.headers["matched"][0]) == n
        for x, key in enumerate(("sojourn", "timer", "ptc")):
            for l, m in enumerate(levels):
                r = max(1, (n * m + 999) // 1000)
                assert n - r + 1 <= pkg.PICK_MAX_K
                pk = host_of(pkg, c, res, a, ((), "largest", key, n - r + 1, X.SERVED))
                assert int(pk.headers["threshold"][0]) == int(sm["q"][x, l]), (c.nUE, key, m)
                if r <= pkg.PICK_MAX_K:
                    pk = host_of(pkg, c, res, a, ((), "smallest", key, r, X.SERVED))
                    assert int(pk.headers["threshold"][0]) == int(sm["q"][x, l]), (c.nUE, key, m)


def test_csv_is_pinned(pkg):
    pk = pkg.Pick(2, (("state", 2, 3),), "largest", "age", 3, X.UNSERVED)
    h, r = pk.headers, pk.rows
    h["nUE"], h["selected"], h["matched"], h["stored"], h["undefined"], h["threshold"], h["ties_left_out"] = [10, 20], [4, 0], [3, 0], [2, 0], [1, 0], [700, -1], [1, 0]
    h["status"] = [0, -5]
    for f, name in enumerate(pkg.UE_FIELDS):
        r[name][0, :2] = [100 + f, -f]
    r["arrival"][0, :2], r["key"][0, :2] = [5, 10], [900, 700]
    cfgs = [pkg.make_cfg(10, seed=3), pkg.make_cfg(20, seed=2 ** 40)]
    assert pkg.pick_csv(pk, cfgs) == (b"10,0,3,10,header,0,4,3,2,1,700,1\n"
                                      b"10,0,3,10,0,900,5,100,101,102,103,104,105,106,107,108,109,110,111,112,113,114,115\n"
                                      b"10,0,3,10,1,700,10,0,-1,-2,-3,-4,-5,-6,-7,-8,-9,-10,-11,-12,-13,-14,-15\n"
                                      b"20,1,1099511627776,20,header,-5,0,0,0,0,-1,0\n")
    assert pkg.pick_csv(pk, labels=["a", "b"]).splitlines()[3] == b"b,1,0,20,header,-5,0,0,0,0,-1,0"
    sp = pk.spec()
    args = (C.byref(sp), pk._headers_ptr(), pk._rows_ptr(0), b"x", 0, 0)
    need = pkg.lib().prach_pick_format_csv(*args, None, 0)
    small = C.create_string_buffer(b"y" * 40, 41)
    assert need > 40 and pkg.lib().prach_pick_format_csv(*args, small, 40) == need and small.value == b""  # does not fit: the length only


def test_refusals_and_argument_errors_need_no_device(pkg, trials, tmp_path):
    c, res, a, _ = trials[0]
    bad_specs = [dict(where=(("state", 3, 2),)), dict(where=(("state", -1, 2),)), dict(where=((9, 0, 1),)), dict(where=((-1, 0, 1),)), dict(where=(("one", 0, 0),) * 5), dict(k=0),
                 dict(k=4097), dict(who=0), dict(who=8), dict(order=3), dict(order=-1), dict(order="index", key="timer"), dict(order="largest", key=9)]
    for kw in bad_specs:
        with pytest.raises(pkg.PrachError) as ei:
            pkg.pick_from_logs([c], [res.steps], [a], **kw)
        assert ei.value.status == -1, kw
    with pytest.raises(pkg.PrachError) as ei:  # the log is not this config's
        pkg.pick_from_logs([c], [res.steps], [a[:-1]])
    assert ei.value.status == -1
    with pytest.raises(pkg.PrachError) as ei:  # NOMA.c logs no trace of a cycle start
        pkg.pick_from_logs([pkg.make_cfg(c.nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX)], [res.steps], [a])
    assert ei.value.status == -2
    # prach_run_trials_pick: spec and variants are judged before the engine is looked at
    L = pkg.lib()
    n = 3
    results = (pkg.PrachResult * n)()

    def call(pk=None, hh=True, rr=True, spec=True, nn=n, variants=(0, 1, 0), reserved=0, unused=0):
        pk = pk or pkg.Pick(n, (("state", 2, 3),), "largest", "age", 16, X.UNSERVED)
        cfgs = (pkg.PrachCfg * n)(*[pkg.make_cfg(100, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s, v in enumerate(variants)])
        sp = pk.spec()
        sp.reserved = reserved
        sp.clause[3].hi = unused
        return L.prach_run_trials_pick(None, cfgs, nn, results, None, C.byref(sp) if spec else None, pk._headers_ptr() if hh else None, pk._rows_ptr() if rr else None)

    assert call() == -1  # everything in order but the engine
    assert call(variants=(0, 2, 1)) == -2  # a NOMA.c trial: refused before anything could be launched
    for bad in (dict(hh=False), dict(rr=False), dict(spec=False), dict(nn=0), dict(reserved=1), dict(unused=7)):
        assert call(**bad) == -1, bad
    for kw in bad_specs:
        assert call(pk=pkg.Pick(n, **kw)) == -1, kw
    assert call(pk=pkg.Pick(n, **bad_specs[0]), variants=(2, 2, 2)) == -1  # a bad spec in a request with a NOMA.c trial is an argument error
    # the sizes: 2^27 words are n x (10 k + 8); the struct layouts; the timing member in front of xtab_ms
    big = 2 ** 27 // (10 * 4096 + 8) + 1
    cfgs = (pkg.PrachCfg * big)(*[pkg.make_cfg(100, rng_mode=pkg.RNG_PHILOX)] * big)
    sp = pkg.Pick(1, k=4096).spec()
    one = pkg.Pick(1, k=1)
    assert L.prach_run_trials_pick(None, cfgs, big, (pkg.PrachResult * big)(), None, C.byref(sp), one._headers_ptr(), one._rows_ptr()) == -2
    assert L.prach_run_trials_pick(None, cfgs, big - 1, (pkg.PrachResult * big)(), None, C.byref(sp), one._headers_ptr(), one._rows_ptr()) == -1
    src = tmp_path / "sz.c"
    src.write_text('#include "prach.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(prach_pick_spec), sizeof(prach_pick_row),'
                   ' _Alignof(prach_pick_row), sizeof(prach_pick), offsetof(prach_pick_row, arrival), sizeof(prach_timing), offsetof(prach_timing, pick_ms),'
                   ' offsetof(prach_timing, xtab_ms), PRACH_PICK_MAX_K, PRACH_PICK_MAX_CLAUSES); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert sizes == [C.sizeof(pkg.PrachPickSpec), 80, 8, C.sizeof(pkg.PrachPick), pkg.PrachPickRow.arrival.offset, C.sizeof(pkg.PrachTiming), pkg.PrachTiming.pick_ms.offset,
                     pkg.PrachTiming.xtab_ms.offset, pkg.PICK_MAX_K, pkg.PICK_MAX_CLAUSES]
    assert sizes[0] == 72 and sizes[3] == 36 and sizes[4] == 64 and sizes[6] + 8 == sizes[7] and pkg.pick_row_dtype().itemsize == 80
    for sym in ("prach_run_trials_pick", "prach_pick_from_logs", "prach_pick_format_csv"):
        assert sym in pkg.EXPORTS


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


GATHER_N, GATHER_K = 11, 5  # trials of the grid: rank 0 holds the odd ones, in descending order; rank 1 the even ones


def _picks(pkg):
    """Synthetic picks: every word of every trial names its trial."""
    rng = np.random.default_rng(9)
    pk = pkg.Pick(GATHER_N, k=GATHER_K)
    for f in pkg.PICK_FIELDS:
        pk.headers[f] = rng.integers(-5, 5000, GATHER_N)
    for f in pk.rows.dtype.names:
        pk.rows[f] = rng.integers(-5, 60000, pk.rows[f].shape)
    return pk


def _same(x, y):
    return x.shape == y.shape and all(np.array_equal(x[f], y[f]) for f in y.dtype.names)


def _gather_worker(rank, world, port, q):
    import importlib
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    distmod = importlib.import_module("nr_randomaccess_amd.dist")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    every = _picks(pkg)
    mine = [k for k in range(GATHER_N) if k % 2 != rank][::-1 if rank == 0 else 1]
    got = distmod.gather_pick_rows(every.headers[mine], every.rows[mine], mine, dst=0)
    q.put((rank, None if got is None else (got[0].tobytes(), got[1].tobytes())))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_pick_rows_two_ranks_gloo(pkg):
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
    every = _picks(pkg)
    assert outs[1] is None  # rank 0 holds every trial, in trial order
    assert _same(np.frombuffer(outs[0][0], dtype=every.headers.dtype), every.headers)
    assert _same(np.frombuffer(outs[0][1], dtype=every.rows.dtype).reshape(GATHER_N, GATHER_K), every.rows)
    # without a process group: the trials in trial order
    order = np.random.default_rng(0).permutation(GATHER_N)
    h, r = distmod.gather_pick_rows(every.headers[order], every.rows[order], order)
    assert _same(h, every.headers) and _same(r, every.rows)
    with pytest.raises(ValueError):
        distmod.gather_pick_rows(every.headers[:3], every.rows[:3], [0, 1])
    with pytest.raises(ValueError):
        distmod.gather_pick_rows(every.headers[:3], every.rows[:2], [0, 1, 2])
