"""Host side of the two per-trial selections over THE NOMA MENU (include/prach.h: prach_noma_summary_from_logs, _stats, _format_csv, prach_noma_pick_from_logs,
_format_csv): the definitions prach::noma_summary_kernel and prach::noma_pick_kernel must equal, against the numpy restatement of
tests/tools/noma_select_ref.py over the ORACLE's UEs, in Philox and in the reference's stream; the statistics against numpy; every argument case of both
specs and every refusal that needs no device; the CLI's refusals.  No GPU."""
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

# (nUE, seed, rng, product kwargs): the input of tests/test_gpu_noma_census.py that populates every state first, then small trials in both streams
ALL_STATES = (2000, 6, "philox", dict(nGrantUL=1, maxMsg2TxCount=3, max_steps=4325))
ALL_STATES_CENSUS = [416, 1547, 13, 2, 1, 12, 5, 4, 0]  # states 0 .. 8, as recorded there
CASES = [ALL_STATES, (1, 4, "philox", {}), (64, 3, "philox", {}), (2000, 1, "philox", {}), (1, 2, "glibc", {}), (64, 5, "glibc", {}),
         (2000, 7, "glibc", dict(max_steps=3000)), (2000, 9, "philox", dict(flags=2))]
# NOMA.c's defaults at 3000 UEs, seed 0, the full 10 000 subframes: in NOMA.c's own rand() stream, and in Philox — the run whose figures README.md and
# profiles/noma_census_kernel.md report (27 stranded, 250 restarted, longest sojourn 237 ms, longest logged timer 52 ms)
FULL_GLIBC, FULL_PHILOX = (3000, 0, "glibc", {}), (3000, 0, "philox", {})
ERR_ARG, ERR_UNSUPPORTED = -1, -2  # PRACH_ERR_ARG, PRACH_ERR_UNSUPPORTED (include/prach.h)

# (fields, who, permille): the default, every field at least once, one field twice, ONE, a field undefined for the class, the extreme levels, 8 levels
SUMMARY_SPECS = [(("sojourn", "timer", "ptc", "lost"), N.SERVED, (500, 950, 990)), (("age",), N.PENDING, (1, 1000)), (("retx", "msg3fail"), N.ALL & ~N.IDLE, (500,)),
                 (("arrival", "completion", "state", "sector"), N.ALL, (250, 500, 750)), (("preamble", "preamble", "one"), N.SERVED | N.DROPPED, (10, 999)),
                 (("sojourn",), N.PENDING, (500, 990)), (("timer",), N.ALL, (1, 125, 250, 375, 500, 625, 750, 1000)), (("state", "age"), N.IDLE, (500,))]
# (where, order, key, k, who)
PICK_SPECS = [((), "index", None, 16, N.ALL), ((("state", 5, 5),), "index", None, 64, N.PENDING), ((), "largest", "sojourn", 10, N.SERVED),
              ((), "smallest", "sojourn", 10, N.SERVED), ((("lost", 1, 2 ** 31 - 1),), "largest", "lost", 300, N.SERVED),
              ((("arrival", 0, 2000), ("ptc", 2, 9), ("sector", 1, 4), ("timer", 10, 60)), "smallest", "timer", 7, N.ALL),
              ((("sojourn", 0, 100000),), "index", None, 5, N.ALL), ((), "largest", "age", 4096, N.PENDING | N.DROPPED), ((), "largest", "state", 1, N.ALL),
              ((("retx", 1, 3),), "smallest", "msg3fail", 33, N.ALL & ~N.IDLE), ((("state", 0, 0),), "index", None, 3, N.IDLE), ((), "smallest", "preamble", 100, N.ALL)]


def product_cfg(pkg, n, seed, rng, kw):
    return pkg.make_cfg(n, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX if rng == "philox" else pkg.RNG_GLIBC, seed=seed, **kw)


def oracle_trial(ob, n, seed, rng, kw):
    okw = dict(kw)
    if "maxMsg2TxCount" in okw:
        okw["maxMsg1ReTx"] = okw.pop("maxMsg2TxCount")
    if "flags" in okw:
        okw["nonsector"] = 1 if okw.pop("flags") & 2 else 0
    res, ues = ob.noma_run_trial(ob.make_noma_cfg(n, **okw), ob.Rng(ob.RNG_PHILOX if rng == "philox" else ob.RNG_GLIBC, seed))
    return res, N.as_array(ues)


@pytest.fixture(scope="module")
def trials(pkg, ob):
    """(product cfg, oracle result, oracle UEs as int32 [nUE, 16], schedule, E) per case, computed once."""
    out = []
    for n, seed, rng, kw in CASES + [FULL_GLIBC, FULL_PHILOX]:
        c = product_cfg(pkg, n, seed, rng, kw)
        res, a = oracle_trial(ob, n, seed, rng, kw)
        out.append((c, res, a, pkg.arrival_schedule(c)[0], min(int(res.steps), 10000)))
    return out


def test_all_states_input_is_the_recorded_one(trials):
    c, res, a, sched, E = trials[0]
    assert (c.nUE, c.seed, c.nGrantUL, c.maxMsg2TxCount, c.max_steps) == (2000, 6, 1, 3, 4325) and E == 4325
    assert N.state_census(a, E) == ALL_STATES_CENSUS


@pytest.mark.parametrize("spec", SUMMARY_SPECS, ids=lambda s: "+".join(s[0]) + f"w{s[1]}q{len(s[2])}")
def test_summary_definition_equals_numpy_on_oracle_ues(pkg, trials, spec):
    fields, who, permille = spec
    for c, res, a, sched, E in trials:
        sm = pkg.noma_summary_from_logs([c], [res.steps], [a], fields, who, permille)
        ref = S.summary(a, sched, c.accessTime, E, fields, who, permille)
        assert S.summary_same(sm.rows, 0, ref), (c.nUE, c.seed, spec, S.summary_describe(sm.rows[0]), S.summary_describe(ref))
        r = sm.rows[0]
        assert int(r["idle"]) + int(r["served"]) + int(r["dropped"]) + int(r["pending"]) == c.nUE and int(r["range_errors"]) == 0
        assert int(r["served"]) == res.nSuccessUE and int(r["dropped"]) == res.raFailedUEs and int(r["idle"]) == c.nUE - res.activeCheck


@pytest.mark.parametrize("spec", PICK_SPECS, ids=lambda s: f"{len(s[0])}cl-{s[1]}-{s[2]}-k{s[3]}-w{s[4]}")
def test_pick_definition_equals_numpy_on_oracle_ues(pkg, trials, spec):
    where, order, key, k, who = spec
    for c, res, a, sched, E in trials:
        pk = pkg.noma_pick_from_logs([c], [res.steps], [a], where, order, key, k, who)
        hdr, rows = S.pick(a, sched, c.accessTime, E, where, order, key, k, who)
        assert S.pick_same(pk, 0, hdr, rows), (c.nUE, c.seed, spec, S.pick_describe(pk, 0), hdr)
        assert hdr["stored"] == min(hdr["matched"], k)


@pytest.mark.parametrize("which", ["rand", "philox"])
def test_the_stranded_ues_of_noma_c_seed_0(pkg, trials, which):
    """Seed 0 at 3000 UEs, in NOMA.c's own rand() stream and in Philox: `where state:5:5, who pending` returns the STRANDED UEs, and its header is the census
    cell of the same logs.  The Philox run is the one README.md reports: 27 of them."""
    c, res, a, sched, E = trials[-2 if which == "rand" else -1]
    assert (c.nUE, c.seed, c.rng_mode, E) == (3000, 0, pkg.RNG_GLIBC if which == "rand" else pkg.RNG_PHILOX, 10000)
    pk = pkg.noma_pick_from_logs([c], [res.steps], [a], [("state", 5, 5)], "index", None, 64, N.PENDING)
    cs = pkg.noma_census_from_logs([c], [res.steps], [a], ("one", 1, 1), ("state", 1, 9), N.PENDING)
    h = pk.headers[0]
    n = N.state_census(a, E)[5]  # counted on the oracle's UEs
    assert int(h["matched"]) == int(h["stored"]) == n == int(cs.cells[0, 0, 5]) > 0 and int(h["selected"]) == int(cs.scalars["selected"][0]) == n
    assert int(h["undefined"]) == 0 == int(cs.scalars["undefined"][0])
    rows = S.pick_rows_of(pk, 0)[:n]
    assert (N.states(rows[:, :16], E) == 5).all() and (np.diff(rows[:, 0]) > 0).all() and not S.pick_rows_of(pk, 0)[n:].any()  # every one stranded, in index order
    assert np.array_equal(rows[:, :16], a[N.states(a, E) == 5])
    if which == "rand":
        return
    assert n == 27
    # the README's other figures: 250 served UEs that started over, a longest sojourn of 237 ms against a longest logged timer of 52 ms
    sm = pkg.noma_summary_from_logs([c], [res.steps], [a], ("sojourn", "timer", "lost"), N.SERVED, (1000,))
    r = sm.rows[0]
    assert (int(r["restarted"]), int(r["pending"]), r["max"].tolist()[:2], r["q"][:2, 0].tolist()) == (250, 27, [237, 52], [237, 52])
    top = pkg.noma_pick_from_logs([c], [res.steps], [a], [], "largest", "sojourn", 1, N.SERVED)
    assert int(top.headers["threshold"][0]) == 237 and int(top.rows[0, 0]["key"]) == 237


def test_all_states_summary_and_a_pick_per_state_agree_with_the_census(pkg, trials):
    c, res, a, sched, E = trials[0]
    cs = pkg.noma_census_from_logs([c], [res.steps], [a], ("one", 1, 1), ("state", 1, 9), N.ALL)
    assert cs.cells[0, 0, :9].tolist() == ALL_STATES_CENSUS
    sm = pkg.noma_summary_from_logs([c], [res.steps], [a], ("state",), N.ALL, (500,))
    r = sm.rows[0]
    assert [int(r[f]) for f in ("idle", "served", "dropped", "pending")] == [int(cs.scalars[f][0]) for f in ("idle", "served", "dropped", "pending")]
    assert int(r["selected"]) == 2000 == int(r["n"][0]) and int(r["sum"][0]) == sum(s * n for s, n in enumerate(ALL_STATES_CENSUS))
    for state in range(9):
        where = cs.cell_clauses(0, state)
        assert where == [(N.ONE, 0, 0), (N.STATE, state, state)]
        pk = pkg.noma_pick_from_logs([c], [res.steps], [a], where, "index", None, 2000, N.ALL)
        n = ALL_STATES_CENSUS[state]
        assert (int(pk.headers["matched"][0]), int(pk.headers["stored"][0]), int(pk.headers["undefined"][0])) == (n, n, 0), state
        assert (N.states(S.pick_rows_of(pk, 0)[:n, :16], E) == state).all()


def test_stats_against_numpy(pkg, trials):
    """Groups with n = 0 and n = 1 among them; a row that is not PRACH_OK and a row with n[x] == 0 are skipped as the header says."""
    sub = trials[:len(CASES)]
    fields, who, permille = ("sojourn", "age", "lost"), N.SERVED | N.PENDING, (500, 990)
    sm = pkg.noma_summary_from_logs([t[0] for t in sub], [t[1].steps for t in sub], [t[2] for t in sub], fields, who, permille)
    sm.rows["status"][5] = -5                   # a trial that failed
    groups = [0, 0, 0, 2, 2, 2, 3, 0]           # group 1 is empty, group 3 has one row, group 2 one good row that is a 1-UE trial
    st = sm.stats(groups, 5)                    # ... and group 4 is empty too
    assert sm.metric_names == ["served_ratio", "dropped_ratio", "pending_ratio", "restart_ratio", "sojourn_mean", "sojourn_p500", "sojourn_p990", "age_mean",
                               "age_p500", "age_p990", "lost_mean", "lost_p500", "lost_p990"] and st.shape == (5, 13)
    rows = sm.rows
    for g in range(5):
        mine = [k for k in range(len(sub)) if groups[k] == g and rows["status"][k] == 0]
        want = [[rows[f][k] / rows["nUE"][k] for k in mine if rows["nUE"][k] > 0] for f in ("served", "dropped", "pending")]
        want.append([rows["restarted"][k] / rows["served"][k] for k in mine if rows["served"][k] > 0])
        for x in range(3):
            have = [k for k in mine if rows["n"][k][x] > 0]
            want.append([rows["sum"][k][x] / rows["n"][k][x] for k in have])
            want += [[float(rows["q"][k][x][l]) for k in have] for l in range(2)]
        for m, xs in enumerate(want):
            ref = S.stats(xs)
            got = st[g, m]
            assert int(got["n"]) == ref[0], (g, m)
            scale = max([1.0] + [abs(v) for v in xs])
            assert np.allclose([got[f] for f in ("mean", "sd", "sem", "min", "max")], ref[1:], rtol=S.STATS_RTOL, atol=S.STATS_RTOL * scale), (g, m, got, ref)
    assert not any(int(st[1, m]["n"]) or st[1, m]["mean"] for m in range(13)) and int(st[3, 0]["n"]) == 1 and st[3, 0]["sd"] == 0.0 == st[3, 0]["sem"]
    # one group without a group array; a NULL group array with ngroups != 1 and a group id out of range are refused
    one = sm.stats()
    assert one.shape == (1, 13) and int(one[0, 0]["n"]) == len(sub) - 1
    L, sp = pkg.lib(), sm.spec()
    out = (pkg.PrachStat * 26)()
    assert L.prach_noma_summary_stats(C.byref(sp), sm._rows_ptr(), len(sub), None, 2, out) == ERR_ARG
    assert L.prach_noma_summary_stats(C.byref(sp), sm._rows_ptr(), len(sub), (C.c_int32 * 8)(0, 0, 0, 0, 0, 0, 0, 2), 2, out) == ERR_ARG
    assert L.prach_noma_summary_stats(C.byref(sp), sm._rows_ptr(), len(sub), (C.c_int32 * 8)(), 1, None) == ERR_ARG


def test_summary_csv_has_the_ci_line_format(pkg, trials):
    sub = trials[:4]
    sm = pkg.noma_summary_from_logs([t[0] for t in sub], [t[1].steps for t in sub], [t[2] for t in sub], ("lost", "ptc"), N.SERVED, (500, 950))
    text = pkg.noma_summary_csv(sm, [0, 1, 0, 1], 2, labels=["a", "b"]).decode()
    lines = text.splitlines()
    st = sm.stats([0, 1, 0, 1], 2)
    assert text.endswith("\n") and len(lines) == 2 * 10
    for g, label in enumerate("ab"):
        for m, name in enumerate(sm.metric_names):
            s = st[g, m]
            assert lines[g * 10 + m] == "%s,%s,%d,%.9g,%.9g,%.9g,%.9g,%.9g" % (label, name, s["n"], s["mean"], s["sd"], s["sem"], s["min"], s["max"])


def test_pick_csv_reuses_the_pick_lines(pkg, trials):
    c, res, a, sched, E = trials[0]
    pk = pkg.noma_pick_from_logs([c], [res.steps], [a], [("state", 2, 7)], "largest", "age", 5, N.ALL)
    text = pkg.noma_pick_csv(pk, [c], labels=["cut"]).decode().splitlines()
    h = pk.headers[0]
    assert text[0] == "cut,0,6,2000,header,0,%d,%d,%d,%d,%d,%d" % tuple(int(h[f]) for f in ("selected", "matched", "stored", "undefined", "threshold", "ties_left_out"))
    assert len(text) == 1 + int(h["stored"]) == 6
    for r, line in enumerate(text[1:]):
        row = S.pick_rows_of(pk, 0)[r]
        assert line == "cut,0,6,2000,%d,%d,%d," % (r, row[17], row[16]) + ",".join(str(int(w)) for w in row[:16])


# ---- arguments and refusals, without an engine ----------------------------------------------------------------------------------------------------------

def summary_spec(pkg, who=1, nfields=2, fields=(2, 12, 0, 0), nq=2, permille=(500, 990, 0, 0, 0, 0, 0, 0), r0=0, r1=0):
    return pkg.PrachNomaSummarySpec(who, nfields, (C.c_int32 * 4)(*fields), nq, (C.c_int32 * 8)(*permille), (C.c_int32 * 2)(r0, r1))


BAD_SUMMARY = [dict(who=0), dict(who=16), dict(who=-1), dict(nfields=0), dict(nfields=5), dict(fields=(13, 0, 0, 0)), dict(fields=(2, -1, 0, 0)),
               dict(fields=(2, 12, 1, 0)), dict(fields=(2, 12, 0, 4)), dict(nq=0), dict(nq=9), dict(permille=(0, 990, 0, 0, 0, 0, 0, 0)),
               dict(permille=(500, 1001, 0, 0, 0, 0, 0, 0)), dict(r0=1), dict(r1=1)]


def pick_spec(pkg, who=15, clauses=((9, 5, 5),), order=0, key=0, k=16, reserved=0, nclauses=None):
    sp = pkg.PrachPickSpec()
    sp.who, sp.nclauses, sp.order, sp.key_field, sp.k, sp.reserved = who, len(clauses) if nclauses is None else nclauses, order, key, k, reserved
    for q, (f, lo, hi) in enumerate(clauses[:4]):
        sp.clause[q] = pkg.PrachPickClause(f, lo, hi)
    return sp


BAD_PICK = [dict(who=0), dict(who=16), dict(who=-1), dict(clauses=((13, 0, 1),)), dict(clauses=((-1, 0, 1),)), dict(clauses=((2, -1, 1),)), dict(clauses=((2, 3, 2),)),
            dict(nclauses=5), dict(nclauses=-1), dict(clauses=((9, 5, 5), (2, 0, 9)), nclauses=1), dict(order=3), dict(order=-1), dict(order=0, key=2),
            dict(order=1, key=13), dict(order=2, key=-1), dict(k=0), dict(k=4097), dict(reserved=1)]


def test_summary_argument_and_refusal_matrix(pkg, trials):
    L = pkg.lib()
    arr = (pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX))
    res = (pkg.PrachResult * 1)()
    rows = np.full(232 // 4, 7, dtype=np.int32)
    rp = rows.ctypes.data_as(C.POINTER(pkg.PrachNomaTrialSummary))

    def call(spec, cfgs=arr, n=1, rows_=rp, res_=res):
        return L.prach_run_trials_noma_summary(None, cfgs, n, res_, None, C.byref(spec) if spec is not None else None, rows_)

    c, ores, a, sched, E = trials[2]
    ptr = a.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
    for bad in BAD_SUMMARY:
        sp = summary_spec(pkg, **bad)
        assert call(sp) == ERR_ARG, bad
        assert L.prach_noma_summary_from_logs(C.byref(sp), C.byref(c), ores.steps, ptr, c.nUE, rp) == ERR_ARG, bad
        assert L.prach_noma_summary_stats(C.byref(sp), rp, 1, None, 1, (pkg.PrachStat * 40)()) == ERR_ARG, bad
        assert L.prach_noma_summary_format_csv(C.byref(sp), (pkg.PrachStat * 40)(), b"x", None, 0) == 0, bad
    good = summary_spec(pkg)
    assert call(None) == ERR_ARG and call(good, rows_=None) == ERR_ARG and call(good, n=0) == ERR_ARG and call(good, cfgs=None) == ERR_ARG and call(good, res_=None) == ERR_ARG
    # the last ids, all four classes, four fields (one twice, ONE) and eight levels are accepted: only the engine is missing
    assert call(summary_spec(pkg, who=15, nfields=4, fields=(12, 12, 0, 9), nq=8, permille=(1, 1000, 2, 3, 4, 5, 6, 7))) == ERR_ARG
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        other = pkg.make_cfg(100, variant=variant, rng_mode=pkg.RNG_PHILOX)
        assert call(good, cfgs=(pkg.PrachCfg * 1)(other)) == ERR_UNSUPPORTED
        assert L.prach_noma_summary_from_logs(C.byref(good), C.byref(pkg.make_cfg(c.nUE, variant=variant, rng_mode=pkg.RNG_PHILOX)), ores.steps, ptr, c.nUE, rp) == ERR_UNSUPPORTED
    assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC))) == ERR_UNSUPPORTED
    two = (pkg.PrachCfg * 2)(arr[0], pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC))
    assert call(good, cfgs=two, n=2, res_=(pkg.PrachResult * 2)()) == ERR_UNSUPPORTED
    assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, flags=2))) == ERR_ARG  # accepted
    assert L.prach_noma_summary_from_logs(C.byref(good), C.byref(c), ores.steps, ptr, c.nUE - 1, rp) == ERR_ARG
    assert L.prach_noma_summary_from_logs(C.byref(good), C.byref(c), ores.steps, ptr, c.nUE, None) == ERR_ARG
    assert (rows == 7).all()  # nothing was written by any refusal
    # the existing summary keeps refusing a NOMA_C cfg
    xs = pkg.Summary(1).spec()
    assert L.prach_run_trials_summary(None, arr, 1, res, None, C.byref(xs), (pkg.PrachTrialSummary * 1)()) == ERR_UNSUPPORTED
    assert L.prach_summary_from_logs(C.byref(xs), C.byref(c), ptr, c.nUE, (pkg.PrachTrialSummary * 1)()) == ERR_UNSUPPORTED


def test_pick_argument_and_refusal_matrix(pkg, trials):
    L = pkg.lib()
    arr = (pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX))
    res = (pkg.PrachResult * 1)()
    hdr = (pkg.PrachPick * 1)()
    rows = np.full(20 * 4096, 7, dtype=np.int32)
    rp = rows.ctypes.data_as(C.POINTER(pkg.PrachPickRow))

    def call(spec, cfgs=arr, n=1, hdr_=hdr, rows_=rp, res_=res):
        return L.prach_run_trials_noma_pick(None, cfgs, n, res_, None, C.byref(spec) if spec is not None else None, hdr_, rows_)

    c, ores, a, sched, E = trials[2]
    ptr = a.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
    for bad in BAD_PICK:
        sp = pick_spec(pkg, **bad)
        assert call(sp) == ERR_ARG, bad
        assert L.prach_noma_pick_from_logs(C.byref(sp), C.byref(c), ores.steps, ptr, c.nUE, hdr, rp) == ERR_ARG, bad
        assert L.prach_noma_pick_format_csv(C.byref(sp), hdr, rp, b"x", 0, 0, None, 0) == 0, bad
    good = pick_spec(pkg)
    assert call(None) == ERR_ARG and call(good, hdr_=None) == ERR_ARG and call(good, rows_=None) == ERR_ARG and call(good, n=0) == ERR_ARG
    assert call(good, cfgs=None) == ERR_ARG and call(good, res_=None) == ERR_ARG
    # the last ids, the DROPPED bit, four clauses and the largest k are accepted: only the engine is missing
    assert call(pick_spec(pkg, who=8, clauses=((12, 0, 5), (11, 0, 63), (10, 0, 5), (9, 0, 8)), order=2, key=12, k=4096)) == ERR_ARG
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=variant, rng_mode=pkg.RNG_PHILOX))) == ERR_UNSUPPORTED
        other = pkg.make_cfg(c.nUE, variant=variant, rng_mode=pkg.RNG_PHILOX)
        assert L.prach_noma_pick_from_logs(C.byref(good), C.byref(other), ores.steps, ptr, c.nUE, hdr, rp) == ERR_UNSUPPORTED
    assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC))) == ERR_UNSUPPORTED
    assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, flags=2))) == ERR_ARG  # accepted
    # the size limit n * k * 10 + n * 8 <= 2^27 words: 3277 trials of k = 4096 are one too many
    n_big = 3277
    assert n_big * (4096 * 10 + 8) > 2 ** 27 >= (n_big - 1) * (4096 * 10 + 8)
    big = (pkg.PrachCfg * n_big)(*[arr[0]] * n_big)
    assert call(pick_spec(pkg, k=4096), cfgs=big, n=n_big, res_=(pkg.PrachResult * n_big)()) == ERR_UNSUPPORTED
    assert call(pick_spec(pkg, k=4096), cfgs=big, n=n_big - 1, res_=(pkg.PrachResult * n_big)()) == ERR_ARG
    assert L.prach_noma_pick_from_logs(C.byref(good), C.byref(c), ores.steps, ptr, c.nUE - 1, hdr, rp) == ERR_ARG
    assert L.prach_noma_pick_from_logs(C.byref(good), C.byref(c), ores.steps, ptr, c.nUE, None, rp) == ERR_ARG
    assert (rows == 7).all()  # nothing was written by any refusal
    # the existing pick keeps refusing a NOMA_C cfg, and a NOMA-only id or bit
    xs = pkg.Pick(1).spec()
    assert L.prach_run_trials_pick(None, arr, 1, res, None, C.byref(xs), hdr, rp) == ERR_UNSUPPORTED
    assert L.prach_pick_from_logs(C.byref(xs), C.byref(c), ores.steps, ptr, c.nUE, hdr, rp) == ERR_UNSUPPORTED
    assert L.prach_run_trials_pick(None, arr, 1, res, None, C.byref(pick_spec(pkg, who=8, clauses=())), hdr, rp) == ERR_ARG


def test_struct_sizes(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "prach.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %d\\n", sizeof(prach_noma_summary_spec),'
                   ' sizeof(prach_noma_trial_summary), offsetof(prach_noma_trial_summary, sum), offsetof(prach_noma_trial_summary, q), sizeof(prach_timing),'
                   ' PRACH_NOMA_SUMMARY_MAX_FIELDS); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    dt = pkg.noma_summary_row_dtype()
    assert got == [C.sizeof(pkg.PrachNomaSummarySpec), dt.itemsize, dt.fields["sum"][1], dt.fields["q"][1], C.sizeof(pkg.PrachTiming), pkg.NOMA_SUMMARY_MAX_FIELDS]
    names = [f[0] for f in pkg.PrachTiming._fields_]
    assert names.index("noma_summary_ms") + 1 == names.index("noma_pick_ms") == names.index("noma_census_ms") - 1
    assert S.MAX_VALUE == pkg.summary_max_value() and pkg.noma_pick_parse_clause("State:5:5") == (N.STATE, 5, 5)


def test_cli_refusals(pkg, tmp_path):
    """--census-ci and --census-pick are refused with a message for another --program, under --rng glibc and next to another reduction, before a device is
    asked for; --ci and --pick keep refusing --program noma with the text they had."""
    out = str(tmp_path / "out.csv")

    def run(*args):
        p = subprocess.run([pkg.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and not os.path.exists(out)
        return p.stdout

    for flag in ("--census-ci", "--census-pick"):
        for program in ("beta", "withnoma"):
            assert flag + " needs --program noma" in run("--program", program, flag, out)
        assert flag + " needs --program noma" in run(flag, out)
        assert flag + " needs --rng philox" in run("--program", "noma", "--rng", "glibc", flag, out)
        for other in ("--census", "--cdf", "--timeline", "--sojourn", "--ci", "--trace", "--xtab", "--pick"):
            assert flag + " cannot be combined" in run("--program", "noma", flag, out, other, str(tmp_path / "other.csv"))
    assert "--census-ci cannot be combined" in run("--program", "noma", "--census-ci", out, "--census-pick", str(tmp_path / "other.csv"))
    assert "--census-ci-who served|pending|dropped|arrived|all" in run("--program", "noma", "--census-ci", out, "--census-ci-who", "idle")
    assert "--census-ci-fields LIST" in run("--program", "noma", "--census-ci", out, "--census-ci-fields", "sojourn,failcount")
    assert "--census-ci-fields LIST" in run("--program", "noma", "--census-ci", out, "--census-ci-fields", "one,one,one,one,one")
    assert "--census-ci-levels LIST" in run("--program", "noma", "--census-ci", out, "--census-ci-levels", "500,1001")
    assert "--census-pick-who served|pending|dropped|arrived|idle|all" in run("--program", "noma", "--census-pick", out, "--census-pick-who", "unserved")
    assert "--census-pick-where FIELD:LO:HI" in run("--program", "noma", "--census-pick", out, "--census-pick-where", "failcount:1:2")
    assert "--census-pick-where FIELD:LO:HI" in run("--program", "noma", "--census-pick", out, "--census-pick-where", "state:5")
    assert "--census-pick-top FIELD or --census-pick-bottom FIELD" in run("--program", "noma", "--census-pick", out, "--census-pick-top", "lost", "--census-pick-bottom", "lost")
    assert "--census-pick-k K" in run("--program", "noma", "--census-pick", out, "--census-pick-k", "4097")
    # the old messages, unchanged
    assert "--ci needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)" in run("--program", "noma", "--ci", out)
    assert "--pick needs --program beta or withnoma (NOMA.c logs no trace of a UE's cycle start)" in run("--program", "noma", "--pick", out)
