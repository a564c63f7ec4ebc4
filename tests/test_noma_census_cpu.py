"""Host side of THE NOMA MENU (include/prach.h, prach_noma_census_*, prach_noma_columns_from_logs): the two definitions prach::noma_census_kernel and
prach::noma_columns_kernel must equal, against the numpy restatement of tests/tools/noma_census_ref.py over the ORACLE's UEs, in Philox and in the
reference's stream; the merge, the CSV text, the quantile through prach_xtab_quantile, and every refusal that needs no device.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_census_ref as N  # noqa: E402

# (nUE, seed, rng, product kwargs): the all-states cut first, then nUE 1, 64 and 2000 in both streams
ALL_STATES = (2000, 6, "philox", dict(nGrantUL=1, maxMsg2TxCount=3, max_steps=4325))
ALL_STATES_CENSUS = [416, 1547, 13, 2, 1, 12, 5, 4, 0]  # states 0 .. 8, counted on the oracle
CASES = [ALL_STATES, (1, 4, "philox", {}), (64, 3, "philox", {}), (2000, 1, "philox", {}), (1, 2, "glibc", {}), (64, 5, "glibc", {}),
         (2000, 7, "glibc", dict(max_steps=3000)), (2000, 9, "philox", dict(flags=2))]
FULL = (3000, 0, "philox", {})  # NOMA.c's defaults over the full 10 000 subframes: the trial of test_full_length_trial_findings
# every field on each axis at least once, widths that do not divide, a 1 x 1 table, overflow bins that are hit (sojourn:7:3, arrival:500:5, timer:1:1)
SPECS = [(("arrival", 500, 20), ("state", 1, 9), N.ALL), (("state", 1, 9), ("arrival", 999, 11), N.ALL), (("one", 1, 1), ("one", 1, 1), N.ALL),
         (("sojourn", 7, 3), ("completion", 333, 31), N.SERVED), (("completion", 1, 65536), ("sojourn", 50, 4), N.SERVED),
         (("timer", 1, 1), ("ptc", 1, 12), N.SERVED | N.PENDING | N.DROPPED), (("ptc", 2, 4), ("timer", 3, 20), N.ALL),
         (("retx", 1, 3), ("msg3fail", 1, 2), N.PENDING | N.DROPPED), (("msg3fail", 1, 4), ("retx", 2, 2), N.SERVED),
         (("age", 13, 700), ("sector", 1, 6), N.IDLE | N.PENDING), (("sector", 2, 3), ("age", 1000, 11), N.DROPPED | N.SERVED),
         (("preamble", 1, 54), ("lost", 5, 40), N.SERVED), (("lost", 1, 1), ("preamble", 10, 5), N.ALL), (("arrival", 500, 5), ("one", 9, 3), N.IDLE | N.DROPPED)]


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
    for n, seed, rng, kw in CASES + [FULL]:
        c = product_cfg(pkg, n, seed, rng, kw)
        res, a = oracle_trial(ob, n, seed, rng, kw)
        sched = pkg.arrival_schedule(c)[0]
        out.append((c, res, a, sched, min(int(res.steps), 10000)))
    return out


def host_census(pkg, c, res, a, spec, **kw):
    return pkg.noma_census_from_logs([c], [res.steps], [a], *spec, **kw)


def test_all_states_input_populates_every_state_and_class(trials):
    c, res, a, sched, E = trials[0]
    assert (c.nUE, c.seed, c.nGrantUL, c.maxMsg2TxCount, c.max_steps) == (2000, 6, 1, 3, 4325) and E == 4325
    assert N.state_census(a, E) == ALL_STATES_CENSUS  # asserted on the oracle's side, before anything is compared
    assert all(N.state_census(a, E)[:8]) and set(np.unique(N.classes(a))) == {N.SERVED, N.PENDING, N.IDLE, N.DROPPED}


def test_schedule_agrees_with_the_oracle(trials):
    """The arrived UEs of the oracle (sector != -1) are exactly the ones the schedule has activated by the last access slot that ran."""
    for c, res, a, sched, E in trials:
        arrived = a[:, N.W_SECTOR] != -1
        assert int(arrived.sum()) == res.activeCheck == sched[(E - 1) // c.accessTime]
        assert arrived[:res.activeCheck].all() and (N.arrivals(c.nUE, sched, c.accessTime)[arrived] < E).all()


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "{}{}x{}{}w{}".format(s[0][0], s[0][2], s[1][0], s[1][2], s[2]))
def test_census_definition_equals_numpy_on_oracle_ues(pkg, trials, spec):
    for c, res, a, sched, E in trials[:len(CASES)]:
        host = host_census(pkg, c, res, a, spec)
        ref = N.census([a], [sched], [c.accessTime], [E], *spec)
        assert N.same(host, ref), (c.nUE, c.seed, spec, N.describe(host), N.describe(ref))
        sc = {f: int(v[0]) for f, v in host.scalars.items()}
        assert int(host.cells.sum()) + sc["undefined"] == sc["selected"] and int(host.cells.sum()) == sc["binned"]
        assert sc["idle"] + sc["served"] + sc["dropped"] + sc["pending"] == sc["ues"] == c.nUE
        assert sc["served"] == res.nSuccessUE and sc["idle"] == c.nUE - res.activeCheck and sc["dropped"] == res.raFailedUEs


def test_every_class_subset(pkg, trials):
    c, res, a, sched, E = trials[0]
    for who in range(1, 16):
        host = host_census(pkg, c, res, a, (("state", 1, 9), ("timer", 10, 30), who))
        assert N.same(host, N.census([a], [sched], [c.accessTime], [E], ("state", 1, 9), ("timer", 10, 30), who)), who
    cls = N.classes(a)
    assert int(host.scalars["selected"][0]) == len(a) and [int((cls == b).sum()) for b in (1, 2, 4, 8)] == \
        [int(host.scalars[f][0]) for f in ("served", "pending", "idle", "dropped")]


def test_overflow_bins_are_hit(pkg, trials):
    c, res, a, sched, E = trials[0]
    h = host_census(pkg, c, res, a, (("arrival", 500, 5), ("timer", 1, 1), N.ALL))
    assert h.cells[0, 5].any() and h.cells[0, 4].any() and h.cells[0, :, 1].any() and h.cells[0, :, 0].any()  # last regular and overflow, on both axes


def test_groups_and_merge_are_order_free(pkg, trials):
    spec = (("arrival", 500, 20), ("state", 1, 9), N.ALL)
    sub = trials[:len(CASES)]
    cfgs, steps, arrays = [t[0] for t in sub], [t[1].steps for t in sub], [t[2] for t in sub]
    groups = [k % 3 for k in range(len(sub))]
    grouped = pkg.noma_census_from_logs(cfgs, steps, arrays, *spec, groups=groups, ngroups=3)
    ref = N.census(arrays, [t[3] for t in sub], [t[0].accessTime for t in sub], [t[4] for t in sub], *spec, groups=groups, ngroups=3)
    assert N.same(grouped, ref)
    single = pkg.noma_census_from_logs(cfgs, steps, arrays, *spec)
    for order in (list(range(len(sub))), list(reversed(range(len(sub)))), [3, 0, 6, 1, 7, 2, 5, 4]):
        m = pkg.NomaCensus(3, *spec)
        for k in order:
            m.merge_group(groups[k], single, k)
        assert m.same_as(grouped), order
    e = pkg.NomaCensus(1, *spec)
    e.merge_group(0, pkg.NomaCensus(1, *spec), 0)
    assert int(e.scalars["row_max"][0]) == -1 and int(e.scalars["col_max"][0]) == -1 and not e.cells.any()


def test_csv_round_trips(pkg, trials):
    c, res, a, sched, E = trials[0]
    spec = (("arrival", 500, 5), ("lost", 20, 4), N.ALL)  # (idle and unserved UEs have no LOST: an `undefined` line)
    h = host_census(pkg, c, res, a, spec)
    text = pkg.noma_census_csv(h, labels=["cut"]).decode()
    cells = np.zeros_like(h.cells[0])
    undefined = 0
    for line in text.splitlines():
        label, r, cc, v = line.split(",")
        assert label == "cut"
        if r == "undefined":
            undefined = int(v)
            continue
        cells[5 if r == "overflow" else int(r) // 500, 4 if cc == "overflow" else int(cc) // 20] = int(v)
    assert text.endswith("\n") and np.array_equal(cells, h.cells[0]) and undefined == int(h.scalars["undefined"][0]) > 0
    # xtab's line format: the same text from an Xtab that holds the same cells
    x = pkg.Xtab(1, ("one", 500, 5), ("one", 20, 4))
    x.cells[:] = h.cells
    x.scalars["undefined"][:] = h.scalars["undefined"]
    assert pkg.xtab_csv(x, labels=["cut"]).decode() == text


def test_quantile_through_prach_xtab_quantile(pkg, trials):
    c, res, a, sched, E = trials[-1]
    qs = (0.0, 1e-9, 0.25, 0.5, 0.95, 0.99, 1.0)
    for spec in ((("arrival", 500, 20), ("sojourn", 5, 60), N.SERVED), (("state", 1, 9), ("timer", 1, 30), N.ALL), (("sector", 1, 6), ("age", 100, 50), N.PENDING)):
        h = host_census(pkg, c, res, a, spec)
        rv, cv = N.values(spec[0][0], a, sched, c.accessTime, E), N.values(spec[1][0], a, sched, c.accessTime, E)
        good = ((N.classes(a) & spec[2]) != 0) & (rv >= 0) & (cv >= 0)
        for row in [-1] + list(range(spec[0][2] + 1)):
            pick = good if row < 0 else good & (np.minimum(rv // spec[0][1], spec[0][2]) == row)
            for q in qs:
                assert h.quantile(0, row, q) == N.rank_quantile(cv[pick], q, spec[1][1], spec[1][2]), (spec, row, q)
    assert h.cell_clauses(2, 50) == [(N.SECTOR, 2, 2), (N.AGE, 5000, 2 ** 31 - 1)]


def test_full_length_trial_findings(pkg, trials):
    """What the census is for: the unserved UEs of NOMA.c's seed-0, 3000-UE run are all STRANDED, and the arrival-to-Msg4 time exceeds the logged timer."""
    c, res, a, sched, E = trials[-1]
    assert (c.nUE, c.seed, E) == (3000, 0, 10000)
    st = N.state_census(a, E)
    h = host_census(pkg, c, res, a, (("one", 1, 1), ("state", 1, 9), N.ALL))
    assert h.cells[0, 0, :9].tolist() == st
    served, pending = int(h.scalars["served"][0]), int(h.scalars["pending"][0])
    assert served + pending == 3000 and st[5] == pending > 0 and st[1] == served  # every pending UE is in state 5
    lost = N.values("lost", a, sched, c.accessTime, E)
    restarted = (N.classes(a) == N.SERVED) & ((a[:, N.W_FAIL] >> 16) > 0)
    assert ((lost > 0) == restarted).all() and restarted.sum() > 0  # LOST > 0 for exactly the restarted UEs
    sj = host_census(pkg, c, res, a, (("sojourn", 1, 1000), ("timer", 1, 1000), N.SERVED))
    assert int(sj.scalars["row_max"][0]) > int(sj.scalars["col_max"][0]) > 0  # max SOJOURN > max TIMER
    print(f"served {served}, stranded {pending}, restarted {int(restarted.sum())}, max sojourn {int(sj.scalars['row_max'][0])}, max timer {int(sj.scalars['col_max'][0])}")


COLUMN_SETS = [N.FIELD_NAMES, ("state",), ("raw:idx", "lost", "raw:failCount", "sector", "sector"), tuple("raw:" + str(w) for w in range(16)),
               ("sojourn", "raw:nowBackoff", "age"), ("preamble", "raw:preambleChange", "one")]


@pytest.mark.parametrize("fields", COLUMN_SETS, ids=lambda f: "+".join(f)[:40])
def test_columns_definition_equals_numpy_on_oracle_ues(pkg, trials, fields):
    names = [f if not f.startswith("raw:") or not f[4:].isdigit() else "raw:" + pkg.UE_FIELDS[int(f[4:])] for f in fields]
    ref_fields = [f if not f.startswith("raw:") or f[4:].isdigit() else "raw:" + str(pkg.UE_FIELDS.index(f[4:])) for f in fields]
    for c, res, a, sched, E in trials[:len(CASES)]:
        col = pkg.noma_columns_from_logs([c], [res.steps], [a], names)
        ref = N.columns(ref_fields, a, sched, c.accessTime, E)
        assert col.data.dtype == np.int32 and np.array_equal(col.data, ref), (c.nUE, c.seed, fields)
        h = col.headers[0]
        cls = N.classes(a)
        assert [int(h[f]) for f in ("idle", "served", "dropped", "pending")] == [int((cls == b).sum()) for b in (N.IDLE, N.SERVED, N.DROPPED, N.PENDING)]


def test_columns_of_several_trials(pkg, trials):
    sub = trials[:4]
    col = pkg.noma_columns_from_logs([t[0] for t in sub], [t[1].steps for t in sub], [t[2] for t in sub], ["state", "arrival"])
    assert col.offsets.tolist() == [0, 2000, 2001, 2065] and col.data.shape == (2, 4065)
    for k, (c, res, a, sched, E) in enumerate(sub):
        assert np.array_equal(col.trial(k), N.columns(["state", "arrival"], a, sched, c.accessTime, E))
    assert np.array_equal(np.bincount(col.column("state")[:2000], minlength=9), ALL_STATES_CENSUS)


ERR_ARG, ERR_UNSUPPORTED = -1, -2  # PRACH_ERR_ARG, PRACH_ERR_UNSUPPORTED (include/prach.h)


# ---- arguments and refusals, without an engine ----------------------------------------------------------------------------------------------------------

def spec_of(pkg, who=15, rf=1, rw=500, rb=20, cf=9, cw=1, cb=9, ngroups=1, r0=0, r1=0):
    return pkg.PrachXtabSpec(who, rf, rw, rb, cf, cw, cb, ngroups, (C.c_int32 * 2)(r0, r1))


BAD_SPECS = [dict(who=0), dict(who=16), dict(who=-1), dict(rf=13), dict(rf=-1), dict(cf=13), dict(rw=0), dict(cw=0), dict(rb=0), dict(rb=65537), dict(cb=0),
             dict(cb=65537), dict(r0=1), dict(r1=1)]


def test_census_argument_and_refusal_matrix(pkg):
    L = pkg.lib()
    noma = pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX)
    arr = (pkg.PrachCfg * 1)(noma)
    res = (pkg.PrachResult * 1)()
    cs = (pkg.PrachNomaCensus * 2)()
    cells = np.full(2 * 21 * 10, 7, dtype=np.uint64)
    cp = cells.ctypes.data_as(C.POINTER(C.c_uint64))

    def call(spec, cfgs=arr, n=1, group=None, cs_=cs, cells_=cp, res_=res):
        return L.prach_run_trials_noma_census(None, cfgs, n, res_, None, C.byref(spec) if spec is not None else None, group, cs_, cells_)

    for bad in BAD_SPECS:
        assert call(spec_of(pkg, **bad)) == ERR_ARG, bad
    assert call(None) == ERR_ARG and call(spec_of(pkg), cs_=None) == ERR_ARG and call(spec_of(pkg), cells_=None) == ERR_ARG
    assert call(spec_of(pkg), n=0) == ERR_ARG and call(spec_of(pkg), cfgs=None) == ERR_ARG and call(spec_of(pkg), res_=None) == ERR_ARG
    assert call(spec_of(pkg, ngroups=0)) == ERR_ARG and call(spec_of(pkg, ngroups=2)) == ERR_ARG  # NULL group with ngroups != n
    assert call(spec_of(pkg, ngroups=2), group=(C.c_int32 * 1)(2)) == ERR_ARG and call(spec_of(pkg, ngroups=2), group=(C.c_int32 * 1)(-1)) == ERR_ARG
    # the last NOMA ids and bits are accepted: with a good spec and no engine the call comes as far as the engine check
    assert call(spec_of(pkg, who=8, rf=12, cf=12)) == ERR_ARG and call(spec_of(pkg, ngroups=2), group=(C.c_int32 * 1)(1)) == ERR_ARG
    # UNSUPPORTED before the engine is looked at: another program, the reference's stream, an oversized table
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        assert call(spec_of(pkg), cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=variant, rng_mode=pkg.RNG_PHILOX))) == ERR_UNSUPPORTED
    assert call(spec_of(pkg), cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC))) == ERR_UNSUPPORTED
    two = (pkg.PrachCfg * 2)(noma, pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC))
    assert call(spec_of(pkg, ngroups=2), cfgs=two, n=2, res_=(pkg.PrachResult * 2)()) == ERR_UNSUPPORTED
    assert call(spec_of(pkg, rb=65536, cb=65536)) == ERR_UNSUPPORTED
    nonsector = pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, flags=2)
    assert call(spec_of(pkg), cfgs=(pkg.PrachCfg * 1)(nonsector)) == ERR_ARG  # accepted: only the engine is missing
    assert (cells == 7).all()  # nothing was written by any refusal


def test_definitions_argument_and_refusal_matrix(pkg, trials):
    L = pkg.lib()
    c, res, a, sched, E = trials[2]
    ptr = a.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
    cs = pkg.PrachNomaCensus()
    cells = np.zeros(21 * 10, dtype=np.uint64)
    cp = cells.ctypes.data_as(C.POINTER(C.c_uint64))
    for bad in BAD_SPECS:
        sp = spec_of(pkg, **bad)
        assert L.prach_noma_census_accumulate_logs(C.byref(sp), C.byref(c), res.steps, ptr, c.nUE, C.byref(cs), cp) == ERR_ARG, bad
    sp = spec_of(pkg)
    assert L.prach_noma_census_accumulate_logs(C.byref(sp), C.byref(c), res.steps, ptr, c.nUE - 1, C.byref(cs), cp) == ERR_ARG
    assert L.prach_noma_census_accumulate_logs(C.byref(sp), C.byref(c), res.steps, ptr, c.nUE, None, cp) == ERR_ARG
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        other = pkg.make_cfg(c.nUE, variant=variant, rng_mode=pkg.RNG_PHILOX)
        assert L.prach_noma_census_accumulate_logs(C.byref(sp), C.byref(other), res.steps, ptr, c.nUE, C.byref(cs), cp) == ERR_UNSUPPORTED
        csp, _ = pkg.noma_columns_spec(["state"])
        out = np.zeros(c.nUE, dtype=np.int32)
        assert L.prach_noma_columns_from_logs(C.byref(csp), C.byref(other), res.steps, ptr, c.nUE, out.ctypes.data, c.nUE) == ERR_UNSUPPORTED
    assert not cells.any() and cs.trials == 0
    # the existing definitions keep refusing a NOMA_C cfg
    xs = pkg.Xtab(1, ("arrival", 500, 20), ("state", 1, 7)).spec()
    assert L.prach_xtab_accumulate_logs(C.byref(xs), C.byref(c), res.steps, ptr, c.nUE, C.byref(pkg.PrachXtab()), cp) == ERR_UNSUPPORTED
    out = np.full(2 * c.nUE, 7, dtype=np.int32)
    for fields, n, stride, want in ((["state"] * 17, c.nUE, c.nUE, ERR_ARG), ([], c.nUE, c.nUE, ERR_ARG), ([13], c.nUE, c.nUE, ERR_ARG), ([32], c.nUE, c.nUE, ERR_ARG),
                                    ([-1], c.nUE, c.nUE, ERR_ARG), (["state"], c.nUE, c.nUE - 1, ERR_ARG), (["state"], c.nUE - 1, c.nUE, ERR_ARG)):
        csp, _ = pkg.noma_columns_spec(fields)
        assert L.prach_noma_columns_from_logs(C.byref(csp), C.byref(c), res.steps, ptr, n, out.ctypes.data, stride) == want, fields
    csp, _ = pkg.noma_columns_spec(["state"])
    csp.reserved[1] = 1
    assert L.prach_noma_columns_from_logs(C.byref(csp), C.byref(c), res.steps, ptr, c.nUE, out.ctypes.data, c.nUE) == ERR_ARG
    assert (out == 7).all()


def test_columns_call_argument_and_refusal_matrix(pkg):
    L = pkg.lib()
    noma = pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX)
    arr = (pkg.PrachCfg * 1)(noma)
    res = (pkg.PrachResult * 1)()
    hdr = (pkg.PrachNomaColumns * 1)()
    out = np.full(300, 7, dtype=np.int32)
    good, _ = pkg.noma_columns_spec(["state", "lost", "raw:failCount"])

    def call(sp, cfgs=arr, hdr_=hdr, out_=out.ctypes.data, cap=100, fn="prach_run_trials_noma_columns"):
        return getattr(L, fn)(None, cfgs, 1, res, None, C.byref(sp) if sp is not None else None, hdr_, out_, cap)

    for fn in ("prach_run_trials_noma_columns", "prach_run_trials_noma_columns_device"):
        assert call(None, fn=fn) == ERR_ARG and call(good, hdr_=None, fn=fn) == ERR_ARG and call(good, out_=None, fn=fn) == ERR_ARG
        for fields in ([13], [32], [-1], [], ["state"] * 17):
            assert call(pkg.noma_columns_spec(fields)[0], fn=fn) == ERR_ARG, fields
        assert call(good, cap=99, fn=fn) == ERR_ARG  # rows_cap below the sum of all nUE
        for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
            assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=variant, rng_mode=pkg.RNG_PHILOX)), fn=fn) == ERR_UNSUPPORTED
        assert call(good, cfgs=(pkg.PrachCfg * 1)(pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)), fn=fn) == ERR_UNSUPPORTED
        assert call(good, cap=(1 << 31) + 1, fn=fn) == ERR_UNSUPPORTED
        assert call(good, fn=fn) == ERR_ARG  # accepted: only the engine is missing
    assert (out == 7).all()
    # the existing columns call keeps refusing a NOMA_C cfg
    xs, _ = pkg.columns_spec(["state"])
    assert L.prach_run_trials_columns(None, arr, 1, res, None, C.byref(xs), (pkg.PrachColumns * 1)(), out.ctypes.data, 100) == ERR_UNSUPPORTED


def test_struct_sizes_and_names(pkg, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include "prach.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %d %d %d %d %d\\n", sizeof(prach_noma_census), sizeof(prach_noma_columns),'
                   ' PRACH_NOMA_NFIELDS, PRACH_NOMA_LOST, PRACH_NOMA_STATE, PRACH_NOMA_DROPPED, PRACH_NOMA_IDLE); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert got == [C.sizeof(pkg.PrachNomaCensus), C.sizeof(pkg.PrachNomaColumns), len(pkg.NOMA_FIELD_NAMES), pkg.NOMA_FIELD_NAMES.index("lost"),
                   pkg.NOMA_FIELD_NAMES.index("state"), pkg.NOMA_DROPPED, pkg.NOMA_IDLE]
    assert pkg.NOMA_FIELD_NAMES == N.FIELD_NAMES and pkg.noma_census_tile_ues() == pkg.xtab_tile_ues()
    assert pkg.NOMA_WHO["all"] == N.ALL and (pkg.NOMA_SERVED, pkg.NOMA_PENDING, pkg.NOMA_IDLE, pkg.NOMA_DROPPED) == (N.SERVED, N.PENDING, N.IDLE, N.DROPPED)


def test_cli_refusals(pkg, tmp_path):
    """--census is refused with a message under --rng glibc, for another --program and next to another reduction, before a device is asked for; the existing
    reductions keep refusing --program noma with the text they had."""
    out = str(tmp_path / "census.csv")

    def run(*args):
        p = subprocess.run([pkg.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and not os.path.exists(out)
        return p.stdout

    assert "--census needs --rng philox" in run("--program", "noma", "--rng", "glibc", "--census", out)
    for program in ("beta", "withnoma"):
        assert "--census needs --program noma" in run("--program", program, "--census", out)
    assert "--census needs --program noma" in run("--census", out)
    for other in ("--cdf", "--timeline", "--sojourn", "--ci", "--trace", "--xtab", "--pick"):
        assert "--census cannot be combined" in run("--program", "noma", "--census", out, other, str(tmp_path / "other.csv"))
    assert "--census-who served|pending|dropped|arrived|all" in run("--program", "noma", "--census", out, "--census-who", "unserved")
    assert "--census-rows FIELD" in run("--program", "noma", "--census", out, "--census-rows", "failcount")
    assert "--census-cols FIELD" in run("--program", "noma", "--census", out, "--census-cols", "state:0")
    assert "--census: too many cells" in run("--program", "noma", "--census", out, "--census-rows", "completion:1:65536", "--census-cols", "age:1:4000")
    assert "--xtab needs --program beta or withnoma" in run("--program", "noma", "--xtab", out)
    assert "--pick needs --program beta or withnoma" in run("--program", "noma", "--pick", out)
