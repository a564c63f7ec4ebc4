"""prach_run_trials_noma_census and prach_run_trials_noma_columns on the GPU: what prach::noma_census_kernel and prach::noma_columns_kernel make on the
device equals, integer for integer, the host definitions on the per-UE logs the same call returns, the numpy restatement of tests/tools/noma_census_ref.py on
those logs, and the same restatement on the ORACLE's UEs: on the input that populates every state, at the tile edges, under every cluster size, in a 48-trial
call, with the cell-wide grouping and the host-built activation table, with and without host logs, under both schemes and under every rerun the engine knows
for NOMA.c (a trial counts once), through the refusals, the timing fields, the device destination and prach_sim --census."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_census_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "tools", "gpu_noma_columns_device_child.py")
CENSUS = (("arrival", 500, 20), ("state", 1, 9), N.ALL)
# every field on an axis, tables with per-wavefront copies, with one copy, and past the LDS window (65537 x 3 cells)
SPECS = [CENSUS, (("one", 1, 1), ("state", 1, 9), N.ALL), (("sojourn", 7, 300), ("lost", 5, 40), N.SERVED), (("timer", 3, 50), ("ptc", 1, 12), N.SERVED | N.PENDING | N.DROPPED),
         (("retx", 1, 3), ("msg3fail", 1, 4), N.PENDING | N.DROPPED), (("sector", 1, 6), ("age", 13, 700), N.ALL), (("preamble", 1, 54), ("completion", 333, 31), N.SERVED),
         (("completion", 1, 65536), ("state", 4, 2), N.ALL), (("age", 1, 4100), ("sector", 2, 3), N.IDLE | N.PENDING), (("lost", 1, 1), ("one", 1, 1), N.ALL)]
COLS = [list(N.FIELD_NAMES), ["raw:" + f for f in ("idx", "timer", "active", "txTime", "firstTxTime", "secondTxTime", "nowBackoff", "preamble", "preambleChange", "rarWindow",
                                                   "maxRarCounter", "preambleTxCounter", "msg2Flag", "connectionRequest", "msg4Flag", "failCount")],
        ["state"], ["age", "raw:failCount", "sector", "sector"]]
ALL_STATES = dict(nUE=2000, seed=6, nGrantUL=1, maxMsg2TxCount=3, max_steps=4325)
ALL_STATES_CENSUS = [416, 1547, 13, 2, 1, 12, 5, 4, 0]


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def noma_cfg(pkg, nUE, seed, **kw):
    return pkg.make_cfg(nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=seed, **kw)


def ref_fields(pkg, fields):
    return [f if not f.startswith("raw:") else "raw:" + str(pkg.UE_FIELDS.index(f[4:])) for f in fields]


def ends(res):
    return [min(int(r.steps), int(r.maxTime)) for r in res]


def numpy_census(pkg, cfgs, arrays, E, spec, grp, ngroups):
    return N.census(arrays, [pkg.arrival_schedule(c)[0] for c in cfgs], [c.accessTime for c in cfgs], E, *spec, groups=grp, ngroups=ngroups)


def census_checked(pkg, eng, cfgs, spec, groups=None, ngroups=None):
    """One call with logs: the device's census equals the host definition and numpy on the logs of the same call, and the identities hold."""
    res, logs, x = eng.run_trials_noma_census(cfgs, *spec, groups=groups, want_logs=True, ngroups=ngroups)
    assert all(r.status == 0 for r in res)
    grp = list(range(len(cfgs))) if groups is None else list(groups)
    host = pkg.noma_census_from_logs(cfgs, [r.steps for r in res], logs, *spec, groups=grp, ngroups=x.ngroups)
    assert x.same_as(host), (spec, N.describe(x), N.describe(host))
    assert N.same(x, numpy_census(pkg, cfgs, [N.as_array(l) for l in logs], ends(res), spec, grp, x.ngroups)), spec
    sc = x.scalars
    assert (x.cells.sum(axis=(1, 2)).astype(np.int64) + sc["undefined"]).tolist() == sc["selected"].tolist() and sc["binned"].tolist() == x.cells.sum(axis=(1, 2)).tolist()
    assert int(sc["served"].sum()) == sum(r.nSuccessUE for r in res) and int(sc["idle"].sum()) == sum(c.nUE - r.activeCheck for c, r in zip(cfgs, res))
    assert int(sc["trials"].sum()) == len(cfgs) and int(sc["ues"].sum()) == sum(c.nUE for c in cfgs) == int((sc["idle"] + sc["served"] + sc["dropped"] + sc["pending"]).sum())
    return res, logs, x


def both_schemes(pkg, eng, cfgs, spec, groups=None, ngroups=None):
    eng.set("xtab_scheme", 0)
    _, _, x0 = census_checked(pkg, eng, cfgs, spec, groups, ngroups)
    eng.set("xtab_scheme", 1)
    res, logs, x1 = census_checked(pkg, eng, cfgs, spec, groups, ngroups)
    assert x1.same_as(x0)
    return res, logs, x1


def columns_checked(pkg, eng, cfgs, fields):
    res, logs, col = eng.run_trials_noma_columns(cfgs, fields, want_logs=True)
    assert all(r.status == 0 for r in res)
    host = pkg.noma_columns_from_logs(cfgs, [r.steps for r in res], logs, fields)
    assert np.array_equal(col.data, host.data) and all(np.array_equal(col.headers[f], host.headers[f]) for f in host.headers.dtype.names), fields
    for k, (c, r, l) in enumerate(zip(cfgs, res, logs)):
        assert np.array_equal(col.trial(k), N.columns(ref_fields(pkg, fields), N.as_array(l), pkg.arrival_schedule(c)[0], c.accessTime, min(int(r.steps), int(r.maxTime)))), (k, fields)
    return res, logs, col


_oracle = {}


def oracle_array(ob, c):
    key = bytes(c)
    if key not in _oracle:
        oc = ob.make_noma_cfg(c.nUE, nPreamble=c.nPreamble, backoff=c.backoff, nGrantUL=c.nGrantUL, maxRarWindow=c.maxRarWindow, maxMsg1ReTx=c.maxMsg2TxCount,
                              accessTime=c.accessTime, max_steps=c.max_steps, cellRadius=c.cellRadius, nonsector=1 if c.flags & 2 else 0)
        res, ues = ob.noma_run_trial(oc, ob.Rng(ob.RNG_PHILOX, c.seed))
        _oracle[key] = (res, N.as_array(ues))
    return _oracle[key]


def equals_oracle(pkg, ob, cfgs, x, spec):
    exp = [oracle_array(ob, c) for c in cfgs]
    assert N.same(x, numpy_census(pkg, cfgs, [a for _, a in exp], [min(int(r.steps), 10000) for r, _ in exp], spec, list(range(len(cfgs))), len(cfgs))), spec


def columns_equal_oracle(pkg, ob, cfgs, col, fields):
    for k, c in enumerate(cfgs):
        r, a = oracle_array(ob, c)
        assert np.array_equal(col.trial(k), N.columns(ref_fields(pkg, fields), a, pkg.arrival_schedule(c)[0], c.accessTime, min(int(r.steps), 10000))), (k, fields)


@pytest.mark.parametrize("cluster", [1, 4, 32])
def test_all_states_input_every_field_and_the_oracle(pkg, ob, eng, cluster):
    """The input that populates every state 0..7 and every class, next to a full-length and a one-UE trial, under cluster sizes 1, 4 and 32."""
    eng.set("cluster", cluster)
    cfgs = [noma_cfg(pkg, ALL_STATES["nUE"], ALL_STATES["seed"], **{k: v for k, v in ALL_STATES.items() if k not in ("nUE", "seed")}), noma_cfg(pkg, 3000, 0), noma_cfg(pkg, 1, 4)]
    r0, a0 = oracle_array(ob, cfgs[0])
    assert N.state_census(a0, 4325) == ALL_STATES_CENSUS  # on the oracle's side, before anything is compared
    for spec in SPECS:
        res, _, x = both_schemes(pkg, eng, cfgs, spec)
        equals_oracle(pkg, ob, cfgs, x, spec)
    _, _, x = census_checked(pkg, eng, cfgs, (("one", 1, 1), ("state", 1, 9), N.ALL))
    assert x.cells[0, 0, :9].tolist() == ALL_STATES_CENSUS
    # the two findings, as the census prints them: every unserved UE of the full-length trial is STRANDED, and the sojourn outlasts the timer
    assert int(x.cells[1, 0, 5]) == int(x.scalars["pending"][1]) == 3000 - res[1].nSuccessUE > 0 and int(x.scalars["dropped"][1]) == 0
    _, _, sj = census_checked(pkg, eng, cfgs[1:2], (("sojourn", 1, 1000), ("timer", 1, 1000), N.SERVED))
    assert int(sj.scalars["row_max"][0]) > int(sj.scalars["col_max"][0]) > 0
    for fields in COLS:
        _, _, col = columns_checked(pkg, eng, cfgs, fields)
        columns_equal_oracle(pkg, ob, cfgs, col, fields)
    assert np.bincount(columns_checked(pkg, eng, cfgs[:1], ["state"])[2].data[0], minlength=9).tolist() == ALL_STATES_CENSUS


def test_trials_around_the_tile_in_one_call(pkg, ob, eng):
    """tile - 1, tile and tile + 1 UEs in one call, cut at 3000 subframes: an odd column offset follows a tile edge, and the last trial has a tile of one UE."""
    tile = pkg.noma_census_tile_ues()
    assert tile == 8192
    cfgs = [noma_cfg(pkg, tile + d, s, max_steps=3000) for s, d in enumerate((-1, 0, 1))]
    for spec in (CENSUS, SPECS[2], SPECS[7], SPECS[8]):
        _, _, x = both_schemes(pkg, eng, cfgs, spec)
    equals_oracle(pkg, ob, cfgs, x, SPECS[8])
    _, _, g = both_schemes(pkg, eng, cfgs, CENSUS, groups=[1, 0, 1])
    assert g.scalars["trials"].tolist() == [1, 2] and int(g.scalars["idle"].sum()) > 0
    for fields in (COLS[0], COLS[3]):
        _, _, col = columns_checked(pkg, eng, cfgs, fields)
        assert col.offsets.tolist() == [0, tile - 1, 2 * tile - 1]
    columns_equal_oracle(pkg, ob, cfgs, col, COLS[3])


def test_a_48_trial_call_with_groups(pkg, eng):
    rng = np.random.default_rng(5)
    cfgs = [noma_cfg(pkg, int(n), k, max_steps=2500 + 100 * (k % 5), nGrantUL=1 + k % 3) for k, n in enumerate(rng.integers(200, 3000, 48))]
    groups = rng.permutation(np.arange(48) % 5).tolist()
    _, _, x5 = both_schemes(pkg, eng, cfgs, CENSUS, groups=groups)
    _, _, per = census_checked(pkg, eng, cfgs, CENSUS)
    merged = pkg.NomaCensus(5, *CENSUS)
    for k, g in enumerate(groups):
        merged.merge_group(g, per, k)
    assert merged.same_as(x5)  # merged on the device == prach_noma_census_merge of the per-trial results
    _, _, x7 = census_checked(pkg, eng, cfgs, SPECS[3], groups=groups, ngroups=7)  # groups 5 and 6 have no trial
    for g in (5, 6):
        assert int(x7.scalars["row_max"][g]) == int(x7.scalars["col_max"][g]) == -1 and not x7.cells[g].any()
    columns_checked(pkg, eng, cfgs, ["state", "lost", "raw:txTime"])


def test_nonsector_flag_and_host_activation(pkg, ob, eng):
    cfgs = [noma_cfg(pkg, 3000, 9, flags=2, max_steps=5000), noma_cfg(pkg, 4097, 10, flags=2, nGrantUL=1, maxMsg2TxCount=3, max_steps=4000)]
    _, _, x = both_schemes(pkg, eng, cfgs, CENSUS)
    equals_oracle(pkg, ob, cfgs, x, CENSUS)
    _, _, col = columns_checked(pkg, eng, cfgs, COLS[0])
    columns_equal_oracle(pkg, ob, cfgs, col, COLS[0])
    plain = [noma_cfg(pkg, 3000, 9, max_steps=5000), noma_cfg(pkg, 2000, 6, nGrantUL=1, maxMsg2TxCount=3, max_steps=4325)]
    _, _, before = census_checked(pkg, eng, plain, CENSUS)
    eng.set("noma_host_activation", 1)
    _, _, after = both_schemes(pkg, eng, plain, CENSUS)
    assert after.same_as(before)
    equals_oracle(pkg, ob, plain, after, CENSUS)
    _, _, col = columns_checked(pkg, eng, plain, COLS[3])
    columns_equal_oracle(pkg, ob, plain, col, COLS[3])


def test_with_and_without_host_logs_and_timing_fields(pkg, eng):
    """The reductions do not need the host's logs; plain results and logs are what they are without them; noma_census_ms and noma_columns_ms are 0 outside
    their own calls, and every other reduction's *_ms is 0 in them."""
    others = ("columns_ms", "pick_ms", "xtab_ms", "trace_ms", "summary_ms", "dist_ms", "timeline_ms", "sojourn_ms")
    cfgs = [noma_cfg(pkg, 3000, 1, max_steps=4000), noma_cfg(pkg, 8193, 2, max_steps=3000), noma_cfg(pkg, 65, 3)]
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    tm = eng.timing()
    assert tm.noma_census_ms == 0 and tm.noma_columns_ms == 0
    exp = pkg.noma_census_from_logs(cfgs, [r.steps for r in res0], logs0, *CENSUS)
    exp_col = pkg.noma_columns_from_logs(cfgs, [r.steps for r in res0], logs0, COLS[0])
    for want in (True, False, [1]):
        res, logs, x = eng.run_trials_noma_census(cfgs, *CENSUS, want_logs=want)
        tm = eng.timing()
        assert x.same_as(exp) and [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert tm.noma_census_ms > 0 and tm.noma_columns_ms == 0 and all(getattr(tm, f) == 0 for f in others)
        assert all(l is None or bytes(l) == bytes(logs0[k]) for k, l in enumerate(logs)) and sum(l is not None for l in logs) == (3 if want is True else 1 if want else 0)
        res, logs, col = eng.run_trials_noma_columns(cfgs, COLS[0], want_logs=want)
        tm = eng.timing()
        assert np.array_equal(col.data, exp_col.data) and [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert tm.noma_columns_ms > 0 and tm.noma_census_ms == 0 and all(getattr(tm, f) == 0 for f in others)
    beta = [pkg.make_cfg(3000, variant=0, rng_mode=pkg.RNG_PHILOX, seed=1)]
    eng.run_trials_xtab(beta)
    tm = eng.timing()
    assert tm.xtab_ms > 0 and tm.noma_census_ms == 0 and tm.noma_columns_ms == 0
    eng.run_trials_dist(cfgs, 64)  # (the one existing reduction that takes NOMA.c trials)
    tm = eng.timing()
    assert tm.dist_ms > 0 and tm.noma_census_ms == 0 and tm.noma_columns_ms == 0


def same_under(pkg, cfgs, *setups):
    """Census and columns of the same call on one fresh engine per setup (None: the call as it is; else a function that sets options), each checked against
    its logs; every setup's outputs equal the first's.  Returns per setup (timing of the census call, timing of the columns call)."""
    out = []
    for fn in setups:
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, x = census_checked(pkg, e, cfgs, CENSUS, groups=[k % 2 for k in range(len(cfgs))] if len(cfgs) > 1 else None)
            t_census = e.timing()
            _, _, col = columns_checked(pkg, e, cfgs, ["state", "lost", "age", "raw:nowBackoff"])
            out.append((x, col, t_census, e.timing()))
        finally:
            e.close()
    a, ca = out[0][:2]
    for b, cb, _, _ in out[1:]:
        assert b.same_as(a) and int(b.scalars["trials"].sum()) == len(cfgs)
        assert np.array_equal(ca.data, cb.data) and all(np.array_equal(ca.headers[f], cb.headers[f]) for f in ca.headers.dtype.names)
    return [(t, tc) for _, _, t, tc in out]


def test_counted_once_ambiguity_rerun(pkg):
    """noma_ambiguity_test = 1: the resolver reports its gain comparisons as ambiguous, the trials are rerun with the host-built table; counted and written once."""
    cfgs = [noma_cfg(pkg, n, s, max_steps=3000) for s, n in enumerate((2000, 4097, 300))]
    (t0, _), (t1, t1c) = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1))
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1c.fallback_trials >= 1 and t1.launches > t0.launches


def test_counted_once_ambiguity_rerun_under_a_split_call(pkg):
    """The same under a memory budget that splits the call: identical to the undisturbed call, and more launches than the ambiguity rerun alone takes."""
    cfgs = [noma_cfg(pkg, 4000, s, max_steps=2500) for s in range(16)]

    def split(e):
        e.set("noma_ambiguity_test", 1)
        e.set("mem_budget_mb", 4)

    (t0, _), (ta, tac), (ts, tsc) = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1), split)
    assert t0.fallback_trials == 0 and ta.fallback_trials >= 1 and ts.fallback_trials >= 1
    assert ts.launches > ta.launches > t0.launches and tsc.launches > tac.launches  # the budget alone forced further launches


def test_e_of_a_trial_that_ends_between_two_slot_heads(pkg, ob, eng):
    """Every UE served at subframe T and max_steps = T + 2 with (T + 1) % accessTime != 0: the kernel runs to max_steps without meeting a slot head, NOMA.c
    breaks behind the last success and prach_result.steps is T + 1.  E is defined from prach_result.steps: AGE = T + 1 - a(i), on a census axis and as a
    column, equals the host definition and the oracle."""
    cfgs = []
    for n in (1, 64):
        for seed in range(16):
            full, _ = oracle_array(ob, noma_cfg(pkg, n, seed))
            T = int(full.steps) - 1
            if full.nSuccessUE == n and (T + 1) % 5 != 0:
                break
        assert full.nSuccessUE == n and (T + 1) % 5 != 0, "no seed among 0..15 ends between two slot heads"
        c = noma_cfg(pkg, n, seed, max_steps=T + 2)
        cut, _ = oracle_array(ob, c)
        assert c.accessTime == 5 and int(cut.steps) == T + 1 and cut.nSuccessUE == n
        cfgs.append(c)
    spec = (("age", 1, 400), ("state", 1, 9), N.ALL)
    res, _, x = both_schemes(pkg, eng, cfgs, spec)
    assert [int(r.steps) for r in res] == [c.max_steps - 1 for c in cfgs]  # not max_steps: the break behind the last success
    equals_oracle(pkg, ob, cfgs, x, spec)
    _, _, col = columns_checked(pkg, eng, cfgs, ["age", "state", "arrival", "completion"])
    columns_equal_oracle(pkg, ob, cfgs, col, ["age", "state", "arrival", "completion"])
    for k, c in enumerate(cfgs):
        age, state, arrival, _ = col.trial(k)
        assert (state == 1).all() and (age == c.max_steps - 1 - arrival).all() and int(x.scalars["row_max"][k]) == int(age.max())  # E = T + 1


def test_refusals_leave_outputs_untouched_and_the_engine_goes_on(pkg, eng):
    import ctypes as C
    L = pkg.lib()
    good = [noma_cfg(pkg, 1000, 1, max_steps=2000), noma_cfg(pkg, 500, 2, max_steps=2000)]
    for bad_cfgs in ([good[0], pkg.make_cfg(1000, variant=0, rng_mode=pkg.RNG_PHILOX)], [good[0], pkg.make_cfg(1000, variant=1, rng_mode=pkg.RNG_PHILOX)],
                     [good[0], pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]):
        n = len(bad_cfgs)
        arr = (pkg.PrachCfg * n)(*bad_cfgs)
        res = (pkg.PrachResult * n)()
        sp = pkg.NomaCensus(n, *CENSUS).spec()
        cs = (pkg.PrachNomaCensus * n)()
        C.memset(cs, 0x5a, C.sizeof(cs))
        cells = np.full(n * 21 * 10, 7, dtype=np.uint64)
        assert L.prach_run_trials_noma_census(eng._h, arr, n, res, None, C.byref(sp), None, cs, cells.ctypes.data_as(C.POINTER(C.c_uint64))) == -2
        assert (cells == 7).all() and bytes(cs) == b"\x5a" * C.sizeof(cs)
        csp, ids = pkg.noma_columns_spec(["state", "lost"])
        hdr = (pkg.PrachNomaColumns * n)()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        out = np.full((2, 2000), 7, dtype=np.int32)
        assert L.prach_run_trials_noma_columns(eng._h, arr, n, res, None, C.byref(csp), hdr, out.ctypes.data, 2000) == -2
        assert (out == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)
    for bad in (dict(who=0), dict(who=16), dict(rows=("arrival", 0, 20)), dict(cols=("state", 1, 65537)), dict(rows=(13, 1, 1)), dict(cols=(-1, 1, 1)), dict(ngroups=3),
                dict(groups=[0, 2], ngroups=2)):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_census(good, **bad)
        assert ei.value.status == -1, bad
    with pytest.raises(pkg.PrachError) as ei:  # 2 x 65537 x 1025 words > 2^27
        eng.run_trials_noma_census(good, ("completion", 1, 65536), ("age", 1, 1024))
    assert ei.value.status == -2
    for fields in ([], ["one"] * 17, [13], [32], [-1]):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_columns(good, fields)
        assert ei.value.status == -1, fields
    # rows behind the sum of nUE keep a sentinel
    n = 2
    arr = (pkg.PrachCfg * n)(*good)
    res = (pkg.PrachResult * n)()
    csp, ids = pkg.noma_columns_spec(["state", "lost"])
    hdr = (pkg.PrachNomaColumns * n)()
    out = np.full((2, 1507), 7, dtype=np.int32)
    assert L.prach_run_trials_noma_columns(eng._h, arr, n, res, None, C.byref(csp), hdr, out.ctypes.data, 1507) == 0
    assert (out[:, 1500:] == 7).all() and (out[0, :1500] >= 0).all() and [h.offset for h in hdr] == [0, 1000]
    census_checked(pkg, eng, good, CENSUS)  # the engine goes on
    columns_checked(pkg, eng, good, ["state", "lost"])
    # the existing kinds keep refusing NOMA.c
    for call in (lambda: eng.run_trials_xtab(good), lambda: eng.run_trials_columns(good, ["state"]), lambda: eng.run_trials_timeline(good, 100, 100)):
        with pytest.raises(pkg.PrachError) as ei:
            call()
        assert ei.value.status == -2


def test_device_destination_in_a_child_process(pkg):
    """torch first: the kernel writes straight into a torch tensor, and torch.bincount of its STATE column is the census's state marginal
    (tests/tools/gpu_noma_columns_device_child.py has the checks)."""
    p = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.returncode, p.stdout[-500:], p.stderr[-3000:])


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_census_equals_the_logs(pkg, eng, tmp_path, workers):
    """prach_sim --program noma --census on a two-point sweep, three seeds per point merged — and the same from two forked workers on one device."""
    out = tmp_path / "census.csv"
    cmd = [pkg.CLI_PATH, "--program", "noma", "-t", "3", "--sweep", "2000:4000:2000", "--out", str(tmp_path), "--census", str(out)]
    spec = CENSUS
    if workers > 1:
        cmd += ["--devices", ",".join(["0"] * workers), "--census-rows", "sector", "--census-cols", "lost:10:30", "--census-who", "served"]
        spec = (("sector", 1, 6), ("lost", 10, 30), N.SERVED)
    else:
        cmd += ["--gpus", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
    points = [2000, 4000]
    cfgs = [noma_cfg(pkg, n, s) for s in range(3) for n in points]
    res, logs = eng.run_trials(cfgs, want_logs=True)
    exp = pkg.noma_census_from_logs(cfgs, [r.steps for r in res], logs, *spec, groups=[k % 2 for k in range(6)], ngroups=2)
    assert out.read_bytes() == pkg.noma_census_csv(exp, labels=points) and len(out.read_bytes()) > 300
