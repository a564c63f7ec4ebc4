"""prach_run_trials_noma_summary and prach_run_trials_noma_pick on the GPU: what prach::noma_summary_kernel and prach::noma_pick_kernel (plus the engine's
sort) make on the device equals, integer for integer, the host definitions on the per-UE logs the same call returns, the numpy restatement of
tests/tools/noma_select_ref.py on those logs, and the same restatement on the ORACLE's UEs: on the input that populates every state, around a block of 1024
UEs, under every cluster size, in a 48-trial call, with the cell-wide grouping and the host-built activation table, with and without host logs, under both
workgroup sizes and under every rerun the engine knows for NOMA.c (a trial is written once); next to the census and the columns of the same cfgs; through
the refusals, the timing fields and prach_sim --census-ci / --census-pick."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_census_ref as N  # noqa: E402
import noma_select_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

# (fields, who, permille)
SUMMARIES = [(("sojourn", "timer", "ptc", "lost"), N.SERVED, (500, 950, 990)), (("age", "state", "retx", "msg3fail"), N.ALL, (1, 500, 1000)),
             (("arrival", "completion", "sector", "preamble"), N.ALL & ~N.IDLE, (250, 750)), (("age", "one", "age"), N.PENDING, (1, 125, 250, 375, 500, 625, 750, 1000)),
             (("sojourn",), N.PENDING | N.IDLE, (500,))]
# (where, order, key, k, who)
PICKS = [((), "index", None, 16, N.ALL), ((("state", 5, 5),), "index", None, 64, N.PENDING), ((), "largest", "sojourn", 10, N.SERVED), ((), "smallest", "sojourn", 10, N.SERVED),
         ((("lost", 1, 2 ** 31 - 1),), "largest", "lost", 300, N.SERVED), ((("arrival", 0, 2000), ("ptc", 2, 9), ("sector", 1, 4), ("timer", 10, 60)), "smallest", "timer", 7, N.ALL),
         ((), "largest", "age", 4096, N.PENDING | N.DROPPED), ((("retx", 1, 3),), "smallest", "msg3fail", 33, N.ALL & ~N.IDLE), ((("state", 0, 0),), "index", None, 3, N.IDLE),
         ((), "smallest", "preamble", 100, N.ALL), ((("sojourn", 0, 100000),), "largest", "state", 1, N.ALL)]
ALL_STATES = dict(nUE=2000, seed=6, nGrantUL=1, maxMsg2TxCount=3, max_steps=4325)
ALL_STATES_CENSUS = [416, 1547, 13, 2, 1, 12, 5, 4, 0]
OTHER_MS = ("noma_census_ms", "noma_columns_ms", "columns_ms", "pick_ms", "xtab_ms", "trace_ms", "summary_ms", "dist_ms", "timeline_ms", "sojourn_ms")


@pytest.fixture
def eng(pkg):
    """An engine of this test's own: whatever option a test sets goes away with it."""
    e = pkg.Engine(0)
    yield e
    e.close()


def noma_cfg(pkg, nUE, seed, **kw):
    return pkg.make_cfg(nUE, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=seed, **kw)


def all_states_cfg(pkg):
    return noma_cfg(pkg, ALL_STATES["nUE"], ALL_STATES["seed"], **{k: v for k, v in ALL_STATES.items() if k not in ("nUE", "seed")})


def trial_data(pkg, cfgs, res, logs):
    """(int32 [nUE, 16], schedule, accessTime, E) per trial, from the logs a call returned."""
    return [(N.as_array(l), pkg.arrival_schedule(c)[0], c.accessTime, min(int(r.steps), int(r.maxTime))) for c, r, l in zip(cfgs, res, logs)]


def summary_checked(pkg, eng, cfgs, spec):
    """One call with logs: the device's rows equal the host definition and numpy on the logs of the same call."""
    res, logs, sm = eng.run_trials_noma_summary(cfgs, *spec, want_logs=True)
    assert all(r.status == 0 for r in res)
    host = pkg.noma_summary_from_logs(cfgs, [r.steps for r in res], logs, *spec)
    assert sm.rows.tobytes() == host.rows.tobytes(), (spec, [S.summary_describe(r) for r in sm.rows[:2]], [S.summary_describe(r) for r in host.rows[:2]])
    for k, (a, sched, at, E) in enumerate(trial_data(pkg, cfgs, res, logs)):
        ref = S.summary(a, sched, at, E, *spec, device=True)
        assert S.summary_same(sm.rows, k, ref), (k, spec, S.summary_describe(sm.rows[k]), S.summary_describe(ref))
        assert int(sm.rows["served"][k]) == res[k].nSuccessUE and int(sm.rows["idle"][k]) == cfgs[k].nUE - res[k].activeCheck
    return res, logs, sm


def pick_checked(pkg, eng, cfgs, spec):
    res, logs, pk = eng.run_trials_noma_pick(cfgs, *spec, want_logs=True)
    assert all(r.status == 0 for r in res)
    host = pkg.noma_pick_from_logs(cfgs, [r.steps for r in res], logs, *spec)
    assert pk.same_as(host), (spec, [S.pick_describe(pk, t) for t in range(min(2, len(cfgs)))], [S.pick_describe(host, t) for t in range(min(2, len(cfgs)))])
    for k, (a, sched, at, E) in enumerate(trial_data(pkg, cfgs, res, logs)):
        hdr, rows = S.pick(a, sched, at, E, *spec, device=True)
        assert S.pick_same(pk, k, hdr, rows), (k, spec, S.pick_describe(pk, k), hdr)
    return res, logs, pk


def both_sizes(pkg, eng, cfgs, spec, kind):
    """The call under both workgroup sizes of its kernel (512 and 1024 threads): identical outputs."""
    fn, opt = (summary_checked, "summary_threads") if kind == "summary" else (pick_checked, "pick_threads")
    eng.set(opt, 512)
    a = fn(pkg, eng, cfgs, spec)[2]
    eng.set(opt, 1024)
    res, logs, b = fn(pkg, eng, cfgs, spec)
    assert b.rows.tobytes() == a.rows.tobytes() and (kind == "summary" or b.same_as(a))
    return res, logs, b


_oracle = {}


def oracle_data(pkg, ob, c):
    """(int32 [nUE, 16], schedule, accessTime, E) of the ORACLE's run of cfg c."""
    key = bytes(c)
    if key not in _oracle:
        oc = ob.make_noma_cfg(c.nUE, nPreamble=c.nPreamble, backoff=c.backoff, nGrantUL=c.nGrantUL, maxRarWindow=c.maxRarWindow, maxMsg1ReTx=c.maxMsg2TxCount,
                              accessTime=c.accessTime, max_steps=c.max_steps, cellRadius=c.cellRadius, nonsector=1 if c.flags & 2 else 0)
        res, ues = ob.noma_run_trial(oc, ob.Rng(ob.RNG_PHILOX, c.seed))
        _oracle[key] = (res, (N.as_array(ues), pkg.arrival_schedule(c)[0], c.accessTime, min(int(res.steps), 10000)))
    return _oracle[key]


def equals_oracle(pkg, ob, cfgs, out, spec, kind):
    for k, c in enumerate(cfgs):
        a, sched, at, E = oracle_data(pkg, ob, c)[1]
        if kind == "summary":
            assert S.summary_same(out.rows, k, S.summary(a, sched, at, E, *spec, device=True)), (k, spec)
        else:
            assert S.pick_same(out, k, *S.pick(a, sched, at, E, *spec, device=True)), (k, spec)


@pytest.mark.parametrize("cluster", [1, 4, 32])
def test_all_states_input_and_the_oracle(pkg, ob, eng, cluster):
    """The input that populates every state 0..7 and every class, next to a full-length and a one-UE trial, under cluster sizes 1, 4 and 32."""
    eng.set("cluster", cluster)
    cfgs = [all_states_cfg(pkg), noma_cfg(pkg, 3000, 0), noma_cfg(pkg, 1, 4)]
    assert N.state_census(oracle_data(pkg, ob, cfgs[0])[1][0], 4325) == ALL_STATES_CENSUS  # on the oracle's side, before anything is compared
    for spec in SUMMARIES:  # (both workgroup sizes under one cluster size: the reducers do not see the simulation's clusters)
        _, _, sm = both_sizes(pkg, eng, cfgs, spec, "summary") if cluster == 1 else summary_checked(pkg, eng, cfgs, spec)
        equals_oracle(pkg, ob, cfgs, sm, spec, "summary")
    for spec in PICKS:
        _, _, pk = both_sizes(pkg, eng, cfgs, spec, "pick") if cluster == 1 else pick_checked(pkg, eng, cfgs, spec)
        equals_oracle(pkg, ob, cfgs, pk, spec, "pick")
    if cluster != 1:
        return
    # the README's findings on the full-length trial, as the two calls print them: 27 stranded, 250 restarted, 237 ms against 52 ms
    _, _, sm = summary_checked(pkg, eng, cfgs, (("sojourn", "timer"), N.SERVED, (1000,)))
    r = sm.rows[1]
    assert (int(r["pending"]), int(r["restarted"]), r["max"][:2].tolist(), r["q"][:2, 0].tolist()) == (27, 250, [237, 52], [237, 52])
    _, _, pk = pick_checked(pkg, eng, cfgs, ((("state", 5, 5),), "index", None, 64, N.PENDING))
    assert int(pk.headers["matched"][1]) == int(pk.headers["stored"][1]) == 27 and (N.states(S.pick_rows_of(pk, 1)[:27, :16], 10000) == 5).all()
    # a pick per state of the all-states trial is the census's state marginal
    for state, n in enumerate(ALL_STATES_CENSUS):
        _, _, pk = pick_checked(pkg, eng, cfgs[:1], ((("state", state, state),), "index", None, 2000, N.ALL))
        assert (int(pk.headers["matched"][0]), int(pk.headers["stored"][0])) == (n, n)


def test_trials_around_a_block_of_1024_in_one_call(pkg, ob, eng):
    """1023, 1024, 1025, 513 and 65 UEs in one call, cut at 3000 subframes: the last block of a trial is full, one short, and one UE."""
    cfgs = [noma_cfg(pkg, n, s, max_steps=3000) for s, n in enumerate((1023, 1024, 1025, 513, 65))]
    for spec in SUMMARIES[:3]:
        _, _, sm = both_sizes(pkg, eng, cfgs, spec, "summary")
    equals_oracle(pkg, ob, cfgs, sm, SUMMARIES[2], "summary")
    for spec in (PICKS[0], PICKS[2], PICKS[5], PICKS[6], ((), "largest", "timer", 1024, N.ALL)):
        _, _, pk = both_sizes(pkg, eng, cfgs, spec, "pick")
    equals_oracle(pkg, ob, cfgs, pk, ((), "largest", "timer", 1024, N.ALL), "pick")


def test_a_48_trial_call_and_the_spread_between_seeds(pkg, eng):
    rng = np.random.default_rng(5)
    cfgs = [noma_cfg(pkg, int(n), k, max_steps=2500 + 100 * (k % 5), nGrantUL=1 + k % 3) for k, n in enumerate(rng.integers(200, 3000, 48))]
    _, _, sm = summary_checked(pkg, eng, cfgs, SUMMARIES[0])
    groups = rng.permutation(np.arange(48) % 5).tolist()
    st = sm.stats(groups, 6)  # group 5 has no trial
    assert st.shape == (6, 4 + 4 * 4) and int(st[5, 0]["n"]) == 0
    for g in range(5):
        mine = [k for k in range(48) if groups[k] == g]
        ref = S.stats([sm.rows["served"][k] / sm.rows["nUE"][k] for k in mine])
        assert int(st[g, 0]["n"]) == ref[0] and np.allclose([st[g, 0][f] for f in ("mean", "sd", "sem", "min", "max")], ref[1:], rtol=S.STATS_RTOL, atol=S.STATS_RTOL)
        have = [k for k in mine if sm.rows["n"][k][0] > 0]
        ref = S.stats([float(sm.rows["q"][k][0][1]) for k in have])  # sojourn_p950
        got = st[g, 4 + 2]
        assert sm.metric_names[6] == "sojourn_p950" and int(got["n"]) == ref[0]
        assert np.allclose([got[f] for f in ("mean", "sd", "sem", "min", "max")], ref[1:], rtol=S.STATS_RTOL, atol=S.STATS_RTOL * max(1.0, ref[5]))
    for spec in (PICKS[1], PICKS[4], PICKS[6]):
        pick_checked(pkg, eng, cfgs, spec)


def test_nonsector_flag_and_host_activation(pkg, ob, eng):
    cfgs = [noma_cfg(pkg, 3000, 9, flags=2, max_steps=5000), noma_cfg(pkg, 4097, 10, flags=2, nGrantUL=1, maxMsg2TxCount=3, max_steps=4000)]
    _, _, sm = summary_checked(pkg, eng, cfgs, SUMMARIES[1])
    equals_oracle(pkg, ob, cfgs, sm, SUMMARIES[1], "summary")
    _, _, pk = pick_checked(pkg, eng, cfgs, PICKS[7])
    equals_oracle(pkg, ob, cfgs, pk, PICKS[7], "pick")
    plain = [noma_cfg(pkg, 3000, 9, max_steps=5000), all_states_cfg(pkg)]
    _, _, sm0 = summary_checked(pkg, eng, plain, SUMMARIES[0])
    _, _, pk0 = pick_checked(pkg, eng, plain, PICKS[4])
    eng.set("noma_host_activation", 1)
    _, _, sm1 = summary_checked(pkg, eng, plain, SUMMARIES[0])
    _, _, pk1 = pick_checked(pkg, eng, plain, PICKS[4])
    assert sm1.rows.tobytes() == sm0.rows.tobytes() and pk1.same_as(pk0)
    equals_oracle(pkg, ob, plain, sm1, SUMMARIES[0], "summary")
    equals_oracle(pkg, ob, plain, pk1, PICKS[4], "pick")


def test_with_and_without_host_logs_and_timing_fields(pkg, eng):
    """The two calls do not need the host's logs; plain results and logs are what they are without them; noma_summary_ms and noma_pick_ms are set in their
    own calls only, and every other reduction's *_ms is 0 in them."""
    cfgs = [noma_cfg(pkg, 3000, 1, max_steps=4000), noma_cfg(pkg, 1025, 2, max_steps=3000), noma_cfg(pkg, 65, 3)]
    res0, logs0 = eng.run_trials(cfgs, want_logs=True)
    tm = eng.timing()
    assert tm.noma_summary_ms == 0 and tm.noma_pick_ms == 0
    exp_sm = pkg.noma_summary_from_logs(cfgs, [r.steps for r in res0], logs0, *SUMMARIES[0])
    exp_pk = pkg.noma_pick_from_logs(cfgs, [r.steps for r in res0], logs0, *PICKS[2])
    for want in (True, False, [1]):
        res, logs, sm = eng.run_trials_noma_summary(cfgs, *SUMMARIES[0], want_logs=want)
        tm = eng.timing()
        assert sm.rows.tobytes() == exp_sm.rows.tobytes() and [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert tm.noma_summary_ms > 0 and tm.noma_pick_ms == 0 and all(getattr(tm, f) == 0 for f in OTHER_MS)
        assert all(l is None or bytes(l) == bytes(logs0[k]) for k, l in enumerate(logs)) and sum(l is not None for l in logs) == (3 if want is True else 1 if want else 0)
        res, logs, pk = eng.run_trials_noma_pick(cfgs, *PICKS[2], want_logs=want)
        tm = eng.timing()
        assert pk.same_as(exp_pk) and [bytes(r) for r in res] == [bytes(r) for r in res0]
        assert tm.noma_pick_ms > 0 and tm.noma_summary_ms == 0 and all(getattr(tm, f) == 0 for f in OTHER_MS)
        assert all(l is None or bytes(l) == bytes(logs0[k]) for k, l in enumerate(logs))
    eng.run_trials_noma_census(cfgs)
    tm = eng.timing()
    assert tm.noma_census_ms > 0 and tm.noma_summary_ms == 0 and tm.noma_pick_ms == 0
    eng.run_trials_pick([pkg.make_cfg(3000, variant=0, rng_mode=pkg.RNG_PHILOX, seed=1)])
    tm = eng.timing()
    assert tm.pick_ms > 0 and tm.noma_summary_ms == 0 and tm.noma_pick_ms == 0


def same_under(pkg, cfgs, *setups):
    """Summary and pick of the same call on one fresh engine per setup (None: the call as it is; else a function that sets options), each checked against its
    logs; every setup's outputs equal the first's.  Returns per setup (timing of the summary call, timing of the pick call)."""
    out = []
    for fn in setups:
        e = pkg.Engine(0)
        try:
            if fn:
                fn(e)
            _, _, sm = summary_checked(pkg, e, cfgs, SUMMARIES[1])
            t_sm = e.timing()
            _, _, pk = pick_checked(pkg, e, cfgs, PICKS[6])
            out.append((sm, pk, t_sm, e.timing()))
        finally:
            e.close()
    for sm, pk, _, _ in out[1:]:
        assert sm.rows.tobytes() == out[0][0].rows.tobytes() and pk.same_as(out[0][1])
    return [(t, tp) for _, _, t, tp in out]


def test_written_once_ambiguity_rerun(pkg):
    """noma_ambiguity_test = 1: the resolver reports its gain comparisons as ambiguous, the trials are rerun with the host-built table; written once, from the rerun."""
    cfgs = [noma_cfg(pkg, n, s, max_steps=3000) for s, n in enumerate((2000, 4097, 300))]
    (t0, _), (t1, t1p) = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1))
    assert t0.fallback_trials == 0 and t1.fallback_trials >= 1 and t1p.fallback_trials >= 1 and t1.launches > t0.launches


def test_written_once_ambiguity_rerun_under_a_split_call(pkg):
    """The same under a memory budget that splits the call: identical to the undisturbed call, and more launches than the ambiguity rerun alone takes."""
    cfgs = [noma_cfg(pkg, 4000, s, max_steps=2500) for s in range(16)]

    def split(e):
        e.set("noma_ambiguity_test", 1)
        e.set("mem_budget_mb", 4)

    (t0, _), (ta, tap), (ts, tsp) = same_under(pkg, cfgs, None, lambda e: e.set("noma_ambiguity_test", 1), split)
    assert t0.fallback_trials == 0 and ta.fallback_trials >= 1 and ts.fallback_trials >= 1
    assert ts.launches > ta.launches > t0.launches and tsp.launches > tap.launches  # the budget alone forced further launches


def test_e_of_a_trial_that_ends_between_two_slot_heads(pkg, ob, eng):
    """Every UE served at subframe T and max_steps = T + 2 with (T + 1) % accessTime != 0: the kernel runs to max_steps without meeting a slot head, NOMA.c
    breaks behind the last success and prach_result.steps is T + 1.  E is defined from prach_result.steps: AGE = T + 1 - a(i), as a summary field and as a
    pick key, equals the host definition and the oracle."""
    cfgs = []
    for n in (1, 64):
        for seed in range(16):
            full = oracle_data(pkg, ob, noma_cfg(pkg, n, seed))[0]
            T = int(full.steps) - 1
            if full.nSuccessUE == n and (T + 1) % 5 != 0:
                break
        assert full.nSuccessUE == n and (T + 1) % 5 != 0, "no seed among 0..15 ends between two slot heads"
        c = noma_cfg(pkg, n, seed, max_steps=T + 2)
        cut = oracle_data(pkg, ob, c)[0]
        assert c.accessTime == 5 and int(cut.steps) == T + 1 and cut.nSuccessUE == n
        cfgs.append(c)
    spec = (("age", "arrival"), N.SERVED, (1, 1000))
    res, _, sm = both_sizes(pkg, eng, cfgs, spec, "summary")
    assert [int(r.steps) for r in res] == [c.max_steps - 1 for c in cfgs]  # not max_steps: the break behind the last success
    equals_oracle(pkg, ob, cfgs, sm, spec, "summary")
    pspec = ((), "largest", "age", 64, N.ALL)
    _, _, pk = both_sizes(pkg, eng, cfgs, pspec, "pick")
    equals_oracle(pkg, ob, cfgs, pk, pspec, "pick")
    for k, c in enumerate(cfgs):
        rows = S.pick_rows_of(pk, k)[:c.nUE]
        assert (rows[:, 17] == c.max_steps - 1 - rows[:, 16]).all() and int(sm.rows["max"][k][0]) == int(rows[0, 17]) == int(sm.rows["q"][k][0][1])  # E = T + 1


def test_agrees_with_the_census_and_the_columns_of_the_same_cfgs(pkg, eng):
    """Class counts against the census's, levels against a sort of the column, `matched` against the cell through NomaCensus.cell_clauses."""
    cfgs = [all_states_cfg(pkg), noma_cfg(pkg, 2500, 3, max_steps=6000)]
    spec = (("sojourn", "lost", "ptc"), N.SERVED, (500, 950, 1000))
    _, _, sm = eng.run_trials_noma_summary(cfgs, *spec)
    _, _, cs = eng.run_trials_noma_census(cfgs, ("arrival", 500, 20), ("state", 1, 9), N.ALL)
    _, _, col = eng.run_trials_noma_columns(cfgs, ["state", "sojourn", "lost", "ptc"])
    for k in range(2):
        assert [int(sm.rows[f][k]) for f in ("idle", "served", "dropped", "pending")] == [int(cs.scalars[f][k]) for f in ("idle", "served", "dropped", "pending")]
        state = col.trial(k)[0]
        for x in range(3):
            v = np.sort(col.trial(k)[1 + x][(state == 1) & (col.trial(k)[1 + x] >= 0)])
            assert int(sm.rows["n"][k][x]) == len(v) and int(sm.rows["sum"][k][x]) == int(v.sum()) and int(sm.rows["max"][k][x]) == int(v[-1])
            assert sm.rows["q"][k][x][:3].tolist() == [int(v[S.rank(len(v), m) - 1]) for m in spec[2]]
        assert int(sm.rows["restarted"][k]) == int(((state == 1) & (col.trial(k)[2] > 0)).sum())
    hit = 0
    for row in (0, 3, 7, 20):
        for state in range(9):
            _, _, pk = eng.run_trials_noma_pick(cfgs, cs.cell_clauses(row, state), "index", None, 4, cs.who)
            assert pk.headers["matched"].tolist() == cs.cells[:, row, state].tolist(), (row, state)
            hit += int(cs.cells[:, row, state].sum() > 0)
    assert hit >= 5  # (cells with UEs among the 36 asked for)


def test_refusals_leave_outputs_untouched_and_the_engine_goes_on(pkg, eng):
    L = pkg.lib()
    good = [noma_cfg(pkg, 1000, 1, max_steps=2000), noma_cfg(pkg, 500, 2, max_steps=2000)]
    for bad_cfgs in ([good[0], pkg.make_cfg(1000, variant=0, rng_mode=pkg.RNG_PHILOX)], [good[0], pkg.make_cfg(1000, variant=1, rng_mode=pkg.RNG_PHILOX)],
                     [good[0], pkg.make_cfg(1000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]):
        n = len(bad_cfgs)
        arr = (pkg.PrachCfg * n)(*bad_cfgs)
        res = (pkg.PrachResult * n)()
        C.memset(res, 0x5a, C.sizeof(res))
        ssp = pkg.NomaSummary(n).spec()
        rows = (pkg.PrachNomaTrialSummary * n)()
        C.memset(rows, 0x5a, C.sizeof(rows))
        assert L.prach_run_trials_noma_summary(eng._h, arr, n, res, None, C.byref(ssp), rows) == -2
        assert bytes(rows) == b"\x5a" * C.sizeof(rows)
        psp = pkg.NomaPick(n, k=4).spec()
        hdr = (pkg.PrachPick * n)()
        prow = (pkg.PrachPickRow * (4 * n))()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        C.memset(prow, 0x5a, C.sizeof(prow))
        assert L.prach_run_trials_noma_pick(eng._h, arr, n, res, None, C.byref(psp), hdr, prow) == -2
        assert bytes(hdr) == b"\x5a" * C.sizeof(hdr) and bytes(prow) == b"\x5a" * C.sizeof(prow) and bytes(res) == b"\x5a" * C.sizeof(res)  # nothing ran
    for bad in (dict(who=0), dict(who=16), dict(fields=()), dict(fields=("one",) * 5), dict(fields=(13,)), dict(fields=(-1,)), dict(permille=()), dict(permille=(0,)),
                dict(permille=(1001,)), dict(permille=(500,) * 9)):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_summary(good, **bad)
        assert ei.value.status == -1, bad
    for bad in (dict(who=0), dict(who=16), dict(where=[(13, 0, 1)]), dict(where=[("state", -1, 1)]), dict(where=[("state", 2, 1)]), dict(where=[("state", 0, 1)] * 5),
                dict(order=3), dict(order="index", key="timer"), dict(order="largest", key=13), dict(k=0), dict(k=4097)):
        with pytest.raises(pkg.PrachError) as ei:
            eng.run_trials_noma_pick(good, **bad)
        assert ei.value.status == -1, bad
    summary_checked(pkg, eng, good, SUMMARIES[0])  # the engine goes on
    pick_checked(pkg, eng, good, PICKS[2])
    # the existing kinds keep refusing NOMA.c
    for call in (lambda: eng.run_trials_summary(good), lambda: eng.run_trials_pick(good)):
        with pytest.raises(pkg.PrachError) as ei:
            call()
        assert ei.value.status == -2


@pytest.mark.parametrize("workers", [1, 2])
def test_cli_census_ci_and_census_pick_equal_the_python_route(pkg, eng, tmp_path, workers):
    """prach_sim --program noma --census-ci / --census-pick on a two-point sweep of three seeds, byte for byte against the Python route — with --gpus 1 and
    from two forked workers on one device."""
    points = [2000, 4000]
    cfgs = [noma_cfg(pkg, n, s) for s in range(3) for n in points]
    base = [pkg.CLI_PATH, "--program", "noma", "-t", "3", "--sweep", "2000:4000:2000", "--out", str(tmp_path)]
    base += ["--gpus", "1"] if workers == 1 else ["--devices", ",".join(["0"] * workers)]
    ci, pick = tmp_path / "ci.csv", tmp_path / "pick.csv"
    if workers == 1:
        ci_args, ci_spec = [], (("sojourn", "timer", "ptc", "lost"), N.SERVED, (500, 950, 990))
        pk_args, pk_spec = ["--census-pick-where", "state:5:5", "--census-pick-who", "pending", "--census-pick-k", "40"], ((("state", 5, 5),), "index", None, 40, N.PENDING)
    else:
        ci_args, ci_spec = ["--census-ci-fields", "age,retx", "--census-ci-who", "arrived", "--census-ci-levels", "10,500,1000"], (("age", "retx"), N.ALL & ~N.IDLE, (10, 500, 1000))
        pk_args = ["--census-pick-where", "lost:1:100000", "--census-pick-where", "sector:0:3", "--census-pick-top", "sojourn", "--census-pick-who", "served"]
        pk_spec = ((("lost", 1, 100000), ("sector", 0, 3)), "largest", "sojourn", 16, N.SERVED)
    subprocess.run(base + ["--census-ci", str(ci)] + ci_args, check=True, stdout=subprocess.DEVNULL, timeout=600)
    subprocess.run(base + ["--census-pick", str(pick)] + pk_args, check=True, stdout=subprocess.DEVNULL, timeout=600)
    _, _, sm = eng.run_trials_noma_summary(cfgs, *ci_spec)
    assert ci.read_bytes() == pkg.noma_summary_csv(sm, [k % 2 for k in range(6)], 2, labels=points) and len(ci.read_bytes()) > 300
    _, _, pk = eng.run_trials_noma_pick(cfgs, *pk_spec)
    assert pick.read_bytes() == pkg.noma_pick_csv(pk, cfgs) and int(pk.headers["stored"].sum()) > 6
