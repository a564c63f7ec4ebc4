"""Host side of NOMA.c's timeline per sector (include/prach.h, prach_noma_timeline_*): the definition prach::noma_timeline_kernel must equal, against the numpy
restatement of tests/tools/noma_timeline_ref.py over the ORACLE's UEs, in Philox and in the reference's stream, cut, cell-wide and full; the identity, the merge,
the CSV text, the structs against a compiled C snippet, every argument and refusal that needs no device, the CLI's refusals and the kernel's symbols.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import noma_census_ref as N  # noqa: E402
import noma_timeline_ref as T  # noqa: E402

# (nUE, seed, rng, product kwargs): the cases of test_noma_census_cpu.py with every class, both streams, the non-sector flag and a cut run
CASES = [(2000, 6, "philox", dict(nGrantUL=1, maxMsg2TxCount=3, max_steps=4325)), (1, 4, "philox", {}), (64, 3, "philox", {}), (2000, 1, "philox", {}),
         (2000, 7, "glibc", dict(max_steps=3000)), (2000, 9, "philox", dict(flags=2))]
# (bins, bin_ms): the trace's default bins over maxTime + 6; non-dividing with both overflows hit; 1 ms; one bin
SPECS = [(2002, 5), (100, 7), (10006, 1), (1, 10006)]
ERR_ARG, ERR_UNSUPPORTED = -1, -2  # PRACH_ERR_ARG, PRACH_ERR_UNSUPPORTED (include/prach.h)


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
    for n, seed, rng, kw in CASES:
        c = product_cfg(pkg, n, seed, rng, kw)
        res, a = oracle_trial(ob, n, seed, rng, kw)
        out.append((c, res, a, pkg.arrival_schedule(c)[0], min(int(res.steps), 10000)))
    return out


def ref_of(trial, bins, bin_ms):
    c, res, a, sched, E = trial
    return T.timeline([a], [sched], [c.accessTime], [E], bins, bin_ms)


def test_inputs_populate_what_the_comparison_needs(trials):
    """Asserted on the oracle's side, before anything is compared."""
    c, res, a, sched, E = trials[0]
    cls = N.classes(a)
    assert set(np.unique(cls)) == {N.SERVED, N.PENDING, N.IDLE, N.DROPPED}
    assert set(np.unique(a[cls != N.IDLE][:, N.W_SECTOR])) == set(range(6))
    full = ref_of(trials[0], 2002, 5)
    assert all(full["series"][T.ARRIVALS, 0, s].sum() > 0 and full["series"][T.SERVED, 0, s].sum() > 0 for s in range(6)) and full["series"][T.DROPPED].sum() > 0
    coarse = ref_of(trials[0], 100, 7)
    assert int(coarse["scalars"]["arrival_overflow"][0]) > 0 and int(coarse["scalars"]["done_overflow"][0]) > 0
    assert set(np.unique(trials[5][2][N.classes(trials[5][2]) != N.IDLE][:, N.W_SECTOR])) == set(range(6))  # the non-sector run logs the UE's own sector


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: f"{s[0]}x{s[1]}ms")
def test_definition_equals_numpy_on_oracle_ues(pkg, trials, spec):
    bins, bin_ms = spec
    for trial in trials:
        c, res, a, sched, E = trial
        host = pkg.noma_timeline_from_logs([c], [res.steps], [a], bins, bin_ms)
        ref = ref_of(trial, bins, bin_ms)
        assert T.same(host, ref), (c.nUE, c.seed, spec, T.describe(host), T.describe(ref))
        assert T.identity(host) and T.identity(ref)
        sc = {f: int(v[0]) for f, v in host.scalars.items()}
        assert sc["ues"] == c.nUE and sc["served"] == res.nSuccessUE and sc["idle"] == c.nUE - res.activeCheck and sc["dropped"] == res.raFailedUEs
        assert sc["undefined"] == 0 and int(host.done.sum()) + sc["done_overflow"] == sc["served"] == int(host.served.sum()) + int((N.classes(a) == N.SERVED)[
            N.arrivals(c.nUE, sched, c.accessTime) // bin_ms >= bins].sum())
        assert int(host.sojourn_sum.sum()) <= sc["sojourn_sum"] and int(host.timer_sum.sum()) <= sc["timer_sum"] <= sc["sojourn_sum"]
        if bins * bin_ms >= 10006:
            assert sc["arrival_overflow"] == sc["done_overflow"] == 0 and int(host.sojourn_sum.sum()) == sc["sojourn_sum"]


def test_pending_per_bin_and_views(pkg, trials):
    c, res, a, sched, E = trials[0]
    tl = pkg.noma_timeline_from_logs([c], [res.steps], [a], 2002, 5)
    assert tl.arrivals.shape == (1, 6, 2002) and tl.arrivals.base is tl.series and tl.done.base is tl.series
    pend = tl.arrivals.astype(np.int64) - tl.served.astype(np.int64) - tl.dropped.astype(np.int64)
    assert (pend >= 0).all() and int(pend.sum()) == int(tl.scalars["pending"][0]) > 0
    for sector in (None, 0, 5):
        arr, sv, dr = tl.named("arrivals", 0, sector), tl.named("served", 0, sector), tl.named("dropped", 0, sector)
        sr, drr, ms, ml = tl.served_ratio(0, sector), tl.dropped_ratio(0, sector), tl.mean_sojourn(0, sector), tl.mean_lost(0, sector)
        arr_, sv_ = np.maximum(arr, 1), np.maximum(sv, 1)  # (the quotients are compared only where the denominator is not 0)
        assert np.array_equal(np.isnan(sr), arr == 0) and np.array_equal(np.isnan(drr), arr == 0) and np.array_equal(np.isnan(ms), sv == 0) and np.array_equal(np.isnan(ml), sv == 0)
        assert np.array_equal(sr[arr > 0], (sv / arr_)[arr > 0]) and np.array_equal(drr[arr > 0], (dr / arr_)[arr > 0])
        ss, ts = tl.named("sojourn_sum", 0, sector), tl.named("timer_sum", 0, sector)
        assert np.array_equal(ms[sv > 0], (ss / sv_)[sv > 0]) and np.array_equal(ml[sv > 0], ((ss - ts) / sv_)[sv > 0]) and (ml[sv > 0] >= 0).all() and (ml[sv > 0] > 0).any()


def test_groups_and_merge_are_order_free(pkg, trials):
    cfgs, steps, arrays = [t[0] for t in trials], [t[1].steps for t in trials], [t[2] for t in trials]
    groups = [k % 3 for k in range(len(trials))]
    grouped = pkg.noma_timeline_from_logs(cfgs, steps, arrays, 100, 7, groups=groups, ngroups=4)
    ref = T.timeline(arrays, [t[3] for t in trials], [t[0].accessTime for t in trials], [t[4] for t in trials], 100, 7, groups=groups, ngroups=4)
    assert T.same(grouped, ref) and T.identity(grouped) and int(grouped.scalars["done_max"][3]) == -1
    single = pkg.noma_timeline_from_logs(cfgs, steps, arrays, 100, 7)
    for order in (list(range(6)), list(reversed(range(6))), [3, 0, 1, 5, 2, 4]):
        m = pkg.NomaTimeline(4, 100, 7)
        for k in order:
            m.merge_group(groups[k], single, k)
        assert m.same_as(grouped), order
    # (a + b) + c == a + (b + c), whole objects
    parts = [pkg.noma_timeline_from_logs([cfgs[k]], [steps[k]], [arrays[k]], 100, 7) for k in (0, 3, 4)]
    fresh = lambda k: pkg.noma_timeline_from_logs([cfgs[k]], [steps[k]], [arrays[k]], 100, 7)
    left = fresh(0).merge(parts[1]).merge(parts[2])
    right = fresh(0).merge(fresh(3).merge(parts[2]))
    assert left.same_as(right) and int(left.scalars["trials"][0]) == 3
    e = pkg.NomaTimeline(1, 100, 7)
    assert e.merge(pkg.NomaTimeline(1, 100, 7)).same_as(pkg.NomaTimeline(1, 100, 7)) and fresh(0).merge(e).same_as(parts[0]) and e.merge(parts[0]).same_as(parts[0])
    with pytest.raises(ValueError):
        e.merge(pkg.NomaTimeline(1, 101, 7))


def filled(pkg):
    a = pkg.NomaTimeline(1, 3, 10)
    a.series[:, 0, 0, 0] = (4, 3, 1, 90, 60, 2)
    a.series[:, 0, 2, 0] = (1, 0, 0, 0, 0, 0)
    a.series[:, 0, 5, 2] = (9, 4, 0, 400, 400, 5)
    for f, v in zip(pkg.NOMA_TIMELINE_FIELDS, (1, 20, 3, 7, 1, 6, 1, 2, 2, 0, 490, 460, 29)):
        a.scalars[f][0] = v
    b = pkg.NomaTimeline(1, 3, 10)
    b.series[:, 0, 0, 0] = (2, 2, 0, 30, 30, 1)
    b.series[:, 0, 1, 1] = (6, 0, 2, 0, 0, 1)
    for f, v in zip(pkg.NOMA_TIMELINE_FIELDS, (2, 11, 0, 2, 2, 4, 0, 0, 0, 3, 30, 30, 31)):
        b.scalars[f][0] = v
    return a, b


CSV = b"""p,arrivals,0,0,6
p,arrivals,2,0,1
p,arrivals,all,0,7
p,arrivals,1,10,6
p,arrivals,all,10,6
p,arrivals,5,20,9
p,arrivals,all,20,9
p,arrivals,all,overflow,2
p,served,0,0,5
p,served,all,0,5
p,served,5,20,4
p,served,all,20,4
p,dropped,0,0,1
p,dropped,all,0,1
p,dropped,1,10,2
p,dropped,all,10,2
p,sojourn_sum,0,0,120
p,sojourn_sum,all,0,120
p,sojourn_sum,5,20,400
p,sojourn_sum,all,20,400
p,timer_sum,0,0,90
p,timer_sum,all,0,90
p,timer_sum,5,20,400
p,timer_sum,all,20,400
p,done,0,0,3
p,done,all,0,3
p,done,1,10,1
p,done,all,10,1
p,done,5,20,5
p,done,all,20,5
p,done,all,overflow,3
"""


def test_merge_and_csv_against_a_literal_block(pkg):
    a, b = filled(pkg)
    ab, ba = filled(pkg)[0].merge(b), filled(pkg)[1].merge(a)
    assert ab.same_as(ba)
    assert [int(ab.scalars[f][0]) for f in pkg.NOMA_TIMELINE_FIELDS] == [3, 31, 3, 9, 3, 10, 1, 2, 2, 3, 520, 490, 31]
    assert pkg.noma_timeline_csv(ab, labels=["p"]) == CSV
    empty = pkg.NomaTimeline(2, 3, 10)
    assert pkg.noma_timeline_csv(empty) == b"" and empty.scalars["done_max"].tolist() == [-1, -1]
    # the line shapes are the trace's: label,series,sector|all,t_ms|overflow,count
    tr = pkg.NomaTrace(1, 3, 10)
    tr.series[0, 0, 2, 1] = 5
    assert pkg.noma_trace_csv(tr, labels=["p"]) == b"p,tx,2,10,5\np,tx,all,10,5\n"
    tl = pkg.NomaTimeline(1, 3, 10)
    tl.series[0, 0, 2, 1] = 5
    assert pkg.noma_timeline_csv(tl, labels=["p"]) == b"p,arrivals,2,10,5\np,arrivals,all,10,5\n"


def test_struct_sizes_offsets_and_timing_tail(pkg, tmp_path):
    src = tmp_path / "sz.c"
    fields = list(pkg.NOMA_TIMELINE_FIELDS)
    offs = ", ".join(f"offsetof(prach_noma_timeline, {f})" for f in fields)
    src.write_text('#include "prach.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){size_t v[] = {sizeof(prach_noma_timeline), sizeof(prach_noma_timeline_spec), '
                   'offsetof(prach_noma_timeline_spec, bins), offsetof(prach_noma_timeline_spec, bin_ms), offsetof(prach_noma_timeline_spec, ngroups), '
                   'offsetof(prach_noma_timeline_spec, reserved), sizeof(prach_timing), offsetof(prach_timing, noma_timeline_ms), offsetof(prach_timing, noma_trace_ms), '
                   'offsetof(prach_timing, sojourn_ms), PRACH_NOMA_TIMELINE_SERIES, PRACH_NOMA_NFIELDS, ' + offs +
                   '}; for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) printf("%zu ", v[i]); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    S, G, TM = pkg.PrachNomaTimelineSpec, pkg.PrachNomaTimeline, pkg.PrachTiming
    assert got == [C.sizeof(G), C.sizeof(S), S.bins.offset, S.bin_ms.offset, S.ngroups.offset, S.reserved.offset, C.sizeof(TM), TM.noma_timeline_ms.offset, TM.noma_trace_ms.offset,
                   TM.sojourn_ms.offset, 6, 13] + [getattr(G, f).offset for f in fields]
    assert C.sizeof(G) == 8 * 13 and TM._fields_[-1][0] == "sojourn_ms" and TM.sojourn_ms.offset + 8 == C.sizeof(TM)  # prach_timing still ends in sojourn_ms
    assert TM.noma_timeline_ms.offset + 8 == TM.noma_trace_ms.offset  # ... and the new field stands in front of noma_trace_ms
    assert pkg.NOMA_TIMELINE_SERIES == T.SERIES and pkg.NOMA_TIMELINE_FIELDS == T.SCALARS and len(pkg.NOMA_FIELD_NAMES) == 13
    assert pkg.noma_timeline_tile_ues() == pkg.timeline_tile_ues() and 1 <= pkg.noma_timeline_window_bins() <= 1024
    # the window, the staged schedule range and the scalars leave room for at least two workgroups on a CU's 160 KiB of LDS
    assert 2 * (4 * (2048 + 36 * pkg.noma_timeline_window_bins()) + 96) <= 160 * 1024


def test_call_argument_and_refusal_matrix(pkg):
    """Spec, groups and variants are judged before the engine is looked at: with engine == NULL every refusal comes, nothing is written, and an acceptable call
    ends with PRACH_ERR_ARG for the missing engine."""
    L = pkg.lib()
    noma = lambda **kw: pkg.make_cfg(500, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=1, **kw)

    def call(cfgs, bins=100, bin_ms=5, ngroups=None, groups=None, reserved=0, null=None, n=None):
        n = len(cfgs) if n is None else n
        ng = len(cfgs) if ngroups is None else ngroups
        tl = pkg.NomaTimeline(max(ng, 1), min(max(bins, 1), 8), bin_ms)
        tl.series[:] = 7
        sp = pkg.PrachNomaTimelineSpec(bins, bin_ms, ng, reserved)
        hdr = (pkg.PrachNomaTimeline * max(ng, 1))()
        C.memset(hdr, 0x5a, C.sizeof(hdr))
        gp = None if groups is None else (C.c_int32 * len(cfgs))(*groups)
        ser = tl._series()
        if null == "series5":
            ser[5] = None
        args = dict(cfgs=(pkg.PrachCfg * len(cfgs))(*cfgs), res=(pkg.PrachResult * len(cfgs))(), spec=C.byref(sp), hdr=hdr, series=ser)
        if null in args:
            args[null] = None
        rc = L.prach_run_trials_noma_timeline(None, args["cfgs"], n, args["res"], None, args["spec"], gp, args["hdr"], args["series"])
        assert (tl.series == 7).all() and bytes(hdr) == b"\x5a" * C.sizeof(hdr)  # nothing is written by a refusal
        return rc

    good = [noma(), noma(flags=2)]  # (PRACH_FLAG_NOMA_NONSECTOR is accepted)
    assert call(good) == ERR_ARG  # (only the engine is missing)
    assert call(good, ngroups=3, groups=[2, 0]) == ERR_ARG and call(good, bins=pkg.TIMELINE_MAX_BINS, bin_ms=1, ngroups=1, groups=[0, 0]) == ERR_ARG  # accepted too
    for kw in (dict(bins=0), dict(bins=-1), dict(bins=pkg.TIMELINE_MAX_BINS + 1), dict(bin_ms=0), dict(bin_ms=-5), dict(ngroups=0), dict(ngroups=-1), dict(ngroups=3),
               dict(ngroups=1), dict(groups=[0, 2], ngroups=2), dict(groups=[-1, 0], ngroups=2), dict(reserved=1), dict(null="cfgs"), dict(null="res"), dict(null="spec"),
               dict(null="hdr"), dict(null="series"), dict(null="series5"), dict(n=0), dict(n=-1)):
        assert call(good, **kw) == ERR_ARG, kw
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        assert call([noma(), pkg.make_cfg(500, variant=variant, rng_mode=pkg.RNG_PHILOX)]) == ERR_UNSUPPORTED
        assert call([pkg.make_cfg(500, variant=variant, rng_mode=pkg.RNG_GLIBC)]) == ERR_UNSUPPORTED
    assert call([noma(), pkg.make_cfg(500, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC)]) == ERR_UNSUPPORTED
    assert call(good, bins=65536, bin_ms=1, ngroups=64, groups=[0, 63]) == ERR_UNSUPPORTED  # 36 x 64 x 65536 words > 2^27
    assert call(good, bins=65536, bin_ms=1, ngroups=56, groups=[0, 55]) == ERR_ARG            # 36 x 56 x 65536 < 2^27: only the engine is missing
    assert call(good, bins=0, ngroups=64, groups=[0, 63]) == ERR_ARG                            # a bad spec comes before UNSUPPORTED
    assert call([noma(), pkg.make_cfg(500, variant=0, rng_mode=pkg.RNG_PHILOX)], bins=0) == ERR_ARG


def test_definition_argument_and_refusal_matrix(pkg, trials):
    L = pkg.lib()
    c, res, a, sched, E = trials[2]
    ptr = a.ctypes.data_as(C.POINTER(pkg.PrachUeLog))
    tl = pkg.NomaTimeline(1, 50, 5)
    hdr = pkg.PrachNomaTimeline()

    def call(sp=None, cfg=c, n=c.nUE, p=ptr, h=hdr, ser=None):
        sp = tl.spec() if sp is None else sp
        return L.prach_noma_timeline_accumulate_logs(C.byref(sp) if sp != "null" else None, C.byref(cfg), res.steps, p, n, C.byref(h) if h is not None else None,
                                                     tl._series(0) if ser is None else ser)

    for bad in (pkg.PrachNomaTimelineSpec(0, 5, 1, 0), pkg.PrachNomaTimelineSpec(pkg.TIMELINE_MAX_BINS + 1, 5, 1, 0), pkg.PrachNomaTimelineSpec(50, 0, 1, 0), "null"):
        assert call(sp=bad) == ERR_ARG
    assert call(n=c.nUE - 1) == ERR_ARG and call(p=None) == ERR_ARG and call(h=None) == ERR_ARG and call(ser=(C.POINTER(C.c_uint64) * 6)()) == ERR_ARG
    for variant in (pkg.VARIANT_BETA_C, pkg.VARIANT_WITHNOMA_C):
        assert call(cfg=pkg.make_cfg(c.nUE, variant=variant, rng_mode=pkg.RNG_PHILOX)) == ERR_UNSUPPORTED
    assert not tl.series.any() and hdr.trials == 0
    assert call() == 0 and hdr.trials == 1 and hdr.ues == c.nUE and hdr.done_max == int(N.values("completion", a, sched, c.accessTime, E).max())
    # the other programs' timeline keeps refusing a NOMA_C cfg
    with pytest.raises(pkg.PrachError) as ei:
        pkg.timeline_from_logs([c], [a], 50, 5)
    assert ei.value.status == ERR_UNSUPPORTED


def test_cli_refusals(pkg, tmp_path):
    """--census-timeline is refused with --census-trace's messages under --rng glibc, for another --program and next to another reduction, before a device is
    asked for."""
    out = str(tmp_path / "tl.csv")

    def run(*args):
        p = subprocess.run([pkg.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and not os.path.exists(out)
        return p.stdout

    assert "--census-timeline needs --rng philox" in run("--program", "noma", "--rng", "glibc", "--census-timeline", out)
    for program in ("beta", "withnoma"):
        assert "--census-timeline needs --program noma" in run("--program", program, "--census-timeline", out)
    assert "--census-timeline needs --program noma" in run("--census-timeline", out)
    for other in ("--cdf", "--timeline", "--sojourn", "--ci", "--trace", "--xtab", "--pick", "--census", "--census-ci", "--census-pick", "--census-trace"):
        assert "--census-timeline cannot be combined with another reduction: one reduction per call" in run("--program", "noma", "--census-timeline", out, other, str(tmp_path / "o.csv"))
    assert "--census-timeline-bin MS" in run("--program", "noma", "--census-timeline", out, "--census-timeline-bin", "0")
    run("--program", "noma", "--timeline", out)  # (the other programs' timeline keeps refusing NOMA.c)


def test_kernel_symbols_and_registers(pkg):
    """The new kernel's device symbols are members of the timeline_kernel family, next to prach::timeline_kernel's own two, in all three libraries; neither
    spills nor uses scratch; and the cut sweep's census of kernel symbols classes them with the reducers without an edit."""
    import isa_registers as I
    import cut_cases
    if not I.tools_present():
        pytest.skip("llvm-objdump / llvm-readobj / c++filt not found")
    for lib in ("libprach_hip.so", "libprach_hip_tinyq.so", "libprach_hip_nobitop3.so"):
        path = os.path.join(os.path.dirname(pkg.LIB_PATH), lib)
        if not os.path.exists(path):
            import __graft_entry__ as g
            g.build()
        meta = I.metadata(path)
        family = sorted(k for k in meta if k.split("<")[0] == "timeline_kernel")
        assert family == ["timeline_kernel<0>", "timeline_kernel<1>", "timeline_kernel<NomaUes, 0>", "timeline_kernel<NomaUes, 1>"], (lib, family)
        for k in family[2:]:
            assert meta[k]["vgpr_spill_count"] == 0 and meta[k]["private_segment_fixed_size"] == 0 and meta[k]["sgpr_spill_count"] == 0, (lib, k, meta[k])
        assert not [b for b in cut_cases.check_symbols(set(meta)) if "timeline_kernel" in b]
