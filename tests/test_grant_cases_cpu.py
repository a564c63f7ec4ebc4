"""The grant sweep's cases without a GPU (tests/tools/grant_cases.py).  From the oracle's grant census alone: switching the census on changes no byte of
any result or log; the oracle's granted set of every subframe of every base is the sorted-prefix definition (the Gr lowest indices, per sector with
sector_grants); the chosen subframes are what the generator yields and hold every class the bases are named for, the exact counts written down here; the
pins are what choose_kernel predicts; every kernel symbol with a grant selection is run by a row; and the cases the suite pinned before hold as many
bin-form subframes as measured when this sweep was added — none, but for one trial.  Conditions on the CASES, not measurements of the library;
tests/test_gpu_grant_sweep.py runs the same cases on the GPU."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cut_cases as CC  # noqa: E402
import grant_cases as GC  # noqa: E402
from kernel_matrix import BETA_CASES  # noqa: E402

# chosen subframes per class over the bases of a row, as counted from the census when the cases were chosen (the census is deterministic: exact)
_PLAIN_PHILOX = dict(ALL=4, CROSS=13, EDGE_GE=15, EDGE_LE=15, ONE=8, LAST=4, W64=4, W65=8)
_PLAIN_GLIBC = dict(ALL=4, CROSS=13, EDGE_GE=15, EDGE_LE=15, ONE=8, LAST=4, W64=4, W65=10)
_SECT_PHILOX = dict(_PLAIN_PHILOX, SECT_CROSS2=2, SECT_W64=2, SECT_W65=2)
_SECT_GLIBC = dict(_PLAIN_GLIBC, SECT_CROSS2=3, SECT_W64=2, SECT_W65=2)
COVERAGE = {
    "batch_w8_philox": _SECT_PHILOX, "batch_w16_philox": _SECT_PHILOX, "legacy_philox": _SECT_PHILOX,
    "batch_glibc": _SECT_GLIBC, "legacy_glibc": _SECT_GLIBC,
    "lcluster4_philox": _PLAIN_PHILOX, "lcluster16_philox": _PLAIN_PHILOX, "cluster4_global_philox": _PLAIN_PHILOX, "cluster4_lds_philox": _PLAIN_PHILOX,
    "lcluster4_glibc": _PLAIN_GLIBC, "lcluster16_glibc": _PLAIN_GLIBC, "cluster_wide_glibc": _PLAIN_GLIBC,
    "cluster_compact_glibc": dict(ALL=4, CROSS=12, EDGE_GE=16, EDGE_LE=16, ONE=8, LAST=4, W64=4, W65=10),
}
# bin-form subframes of the whole trial (ns > 64 with a grant left; per-sector: ns > 64) per (base, variant), Philox / rand()
BIN_FORM = {
    ("g6_16384", 0): (1189, 1197), ("g6_16384", 1): (1199, 1190), ("g12_16385", 0): (262, 300), ("g12_16385", 1): (261, 266),
    ("g2_16000", 0): (1334, 1315), ("g2_16000", 1): (1327, 1322), ("g128_48000", 0): (26, 35), ("g128_48000", 1): (26, 33),
    ("sect_g3_16384", 1): (143, 164),
}

# The cases the suite pinned to a kernel, or stopped at consecutive subframes, before this sweep: (the most singleton callers of a subframe, bin-form
# subframes) per (variant, RNG mode 1 / 0), with the seeds those suites use.  The gap the grant sweep closes, on record.
_NONE = {(0, 1): 0, (0, 0): 0, (1, 1): 0, (1, 0): 0}
EXISTING = {
    # gpu_kernel_matrix.py (seed 100 k + variant)
    "matrix:corner_1500": _NONE, "matrix:default_3000": _NONE, "matrix:p8_at1": _NONE, "matrix:p3_b40_at6": _NONE, "matrix:p1_msg2_1": _NONE,
    "matrix:default_16000": {(0, 1): 0, (0, 0): 0, (1, 1): 17, (1, 0): 27},  # (leaves lcluster4_philox; 72 / 79 singleton callers at the most)
    # cut_cases.BETA_BASES (seed 700 + 10 k + variant): the cut sweep, and at7_g3_2500 the quiet and roles sweeps
    "cut:default_1500": _NONE, "cut:at7_g3_2500": _NONE, "cut:at2_g3_2000": _NONE, "cut:corner_1500": _NONE, "cut:default_64": _NONE,
}
EXISTING_MOST = 17  # singleton callers in one subframe, over every case above but default_16000
# tests/test_gpu_parity.py test_gpu_equals_oracle (seed 5, kernel not pinned): where the bin form did run, somewhere in 10 000 subframes
UNPINNED = {(0, 20000): (0, 0), (1, 20000): (756, 750), (1, 30000): (1325, 1333)}


def _existing_trials():
    out = []
    for k, (name, n, kw) in enumerate(BETA_CASES):
        if f"matrix:{name}" in EXISTING:
            out += [(f"matrix:{name}", ("beta", v, n, kw, r, 100 * k + v)) for v in (0, 1) for r in (1, 0)]
    for k, (name, n, kw) in enumerate(CC.BETA_BASES):
        out += [(f"cut:{name}", ("beta", v, n, kw, r, 700 + 10 * k + v)) for v in (0, 1) for r in (1, 0)]
    return out


def _unpinned_trials():
    return [((v, n), ("beta", v, n, {}, r, 5)) for v, n in UNPINNED for r in (1, 0)]


@pytest.fixture(scope="module")
def censused():
    """The grant census of every distinct base trial (both variants, both RNG modes, the compact row's 65 preambles) and of the earlier cases, once."""
    GC.census_many([t for t, _ in GC.distinct_bases().values()] + [t for _, t in _existing_trials()] + [t for _, t in _unpinned_trials()])
    return True


@pytest.mark.parametrize("rng", [0, 1])
def test_census_changes_no_result(ob, rng):
    """Every counter, every logged field of every UE and the formatted Results / Logs text of a trial are the same bytes with the census on and off: both
    variants, the per-sector budgets, a trial cut short, and a base of the sweep."""
    cases = [(0, 3000, {}), (1, 3000, {}), (1, 3000, dict(nGrantUL=3, sector_grants=1)), (0, 2500, dict(accessTime=7, nGrantUL=3, nPreamble=20, max_steps=4001)),
             (1, 16384, dict(nPreamble=16, nGrantUL=6, max_steps=4000))]
    for v, n, kw in cases:
        cfg = ob.make_cfg(n, variant=v, **kw)
        res0, ues0 = ob.run_trial(cfg, ob.Rng(rng, 700 + v))
        res1, ues1, cen = ob.run_trial_grant_census(cfg, ob.Rng(rng, 700 + v))
        res2, ues2 = ob.run_trial(cfg, ob.Rng(rng, 700 + v))  # (and off again afterwards)
        assert bytes(res0) == bytes(res1) == bytes(res2) and bytes(ues0) == bytes(ues1) == bytes(ues2), (v, n, kw)
        assert ob.format_logs(ues0, n) == ob.format_logs(ues1, n) and ob.format_results(cfg, res0) == ob.format_results(cfg, res1)
        # the census itself: every singleton call of the trial, none twice (txop - collisions counts them: a single adds 1 to txop only)
        assert int(cen["ns"].sum()) == len(cen["idx"]) == res0.totalPreambleTxop - res0.collisionPreambles
        assert (np.diff(cen["t"]) > 0).all() and (cen["ns"] > 0).all()


def test_definition_equals_the_oracle_in_every_subframe(censused):
    """Sort the singleton callers' indices, take the first Gr (per sector: the first of each sector's budget): the oracle's granted set, in every subframe of
    every base, both variants, both RNG modes."""
    n = 0
    for (tag, rng), (t, _) in sorted(GC.distinct_bases().items()):
        bad = GC.check_definition(t)
        assert not bad, (tag, rng, bad[:3])
        n += len(GC.census(t)["sub"])
    assert n > 60000  # (subframes with a singleton call: 65 740 when the cases were chosen)
    # the definition, on a hand-made subframe: scan order is not assumed
    assert GC.definition([9, 3, 7, 1], 2).tolist() == [False, True, False, True] and not GC.definition([5, 6], 0).any() and GC.definition([5, 6], 9).all()
    assert GC.definition_sectors(np.array([9, 3, 7, 1]), np.array([0, 0, 5, 5]), [1, 0, 0, 0, 0, 0]).tolist() == [False, True, False, False]
    assert [GC.binshift(n) for n in (1, 1024, 1025, 16000, 16384, 16385, 48000, 65536, 65537)] == [0, 0, 1, 4, 4, 5, 6, 6, 7]


def test_classes_on_hand_made_subframes():
    """classify() on subframes written by hand (16 384 UEs: bins of 16): one class at a time."""
    far = np.arange(100, 100 + 16 * 70, 16)  # 70 callers, one per bin
    assert GC.classify(16384, 70, 5, far) == {"EDGE_LE", "EDGE_GE"}                  # (bins of one caller: bin 5 ends at exactly 5, bin 6 starts there)
    assert GC.classify(16384, 70, 70, far) == {"ALL", "EDGE_LE"} and GC.classify(16384, 70, 99, far) == {"ALL"}
    assert GC.classify(16384, 70, 1, far) == {"ONE", "EDGE_LE", "EDGE_GE"} and GC.classify(16384, 70, 0, far) == set()
    pair = np.concatenate([[0, 1, 2], far])                                            # bin 0 holds three callers
    assert GC.classify(16384, 73, 2, pair) == {"CROSS"} and GC.classify(16384, 73, 3, pair) == {"EDGE_LE", "EDGE_GE"}
    last = np.concatenate([far, [16383]])                                              # a caller in bin 1023 behind 70 others: past a budget of 5, inside one of 71
    assert GC.classify(16384, 71, 5, last) == {"EDGE_LE", "EDGE_GE", "LAST"} and GC.classify(16384, 71, 70, last) == {"EDGE_LE", "EDGE_GE", "LAST"}
    assert GC.classify(16384, 71, 71, last) == {"ALL", "EDGE_LE", "LAST", "TOP"} and not {"LAST", "TOP"} & GC.classify(16385, 71, 71, np.concatenate([far, [16384]]))
    pack = np.concatenate([far[:60], 16368 + np.arange(10)])                           # ten callers in bin 1023 behind 60: a budget of 65 crosses in the last bin
    assert GC.classify(16384, 70, 65, pack) == {"CROSS", "LAST", "TOP"} and GC.classify(16384, 70, 60, pack) == {"EDGE_LE", "EDGE_GE", "LAST"}
    assert GC.classify(16384, 64, 5, far[:64]) == {"W64"} and GC.classify(16384, 65, 5, far[:65]) == {"W65", "EDGE_LE", "EDGE_GE"}
    two = np.concatenate([[0, 1, 2, 3, 4, 5, 6, 7], far[8:]])                          # four callers of sector 0 and four of sector 1, all in the first bin of 128 UEs
    sec = np.concatenate([[0] * 4, [1] * 4, 2 + np.arange(62) % 4])
    assert GC.classify(16384, 70, 0, two, sec, [2, 2, 0, 0, 0, 0]) == {"SECT_CROSS2", "SECT_SPENT"}
    assert GC.classify(16384, 70, 0, two, sec, [2, 0, 0, 0, 0, 0]) == {"SECT_SPENT"} and GC.classify(16384, 70, 0, two, sec, [0] * 6) == set()
    assert GC.classify(16384, 70, 0, two, sec, [2, 2, 20, 20, 20, 20]) == {"SECT_CROSS2"}


def test_chosen_subframes_are_what_the_generator_yields(censused):
    """CHOSEN is choose() of every base; every base holds each class it is named for PER_CLASS times among its chosen subframes; at most MAX_CUTS cuts."""
    want = {k: GC.choose(t, named) for k, (t, named) in GC.distinct_bases().items()}
    assert want == GC.CHOSEN
    for (tag, rng), (t, named) in GC.distinct_bases().items():
        cl = GC.classes_of(t)
        for c in named:
            assert sum(c in cl[tt] for tt in GC.CHOSEN[(tag, rng)]) >= GC.PER_CLASS, (tag, rng, c)
        cuts = GC.cuts_of(tag, rng)
        assert 0 < len(cuts) <= GC.MAX_CUTS and max(cuts) <= int(GC.census(t)["res"].steps), (tag, rng)
    # Within a base Gr is nGrantUL - 1 in every bin-form subframe (a window's first loaded subframe uses the budget up, and the preference of choose() for
    # another number of grants left finds none); the bases differ: 1, 5, 11 and 127 grants left
    left = {}
    for (tag, rng), (t, _) in GC.distinct_bases().items():
        if not t[3].get("sector_grants"):
            left.setdefault(rng, set()).update(int(lf) for tt, ns, lf, *_ in GC.census(t)["sub"] if ns > GC.WAVE and lf > 0)
    assert left == {0: {1, 5, 11, 127}, 1: {1, 5, 11, 127}}


@pytest.mark.parametrize("row", [r["name"] for r in GC.GRANT_ROWS])
def test_row_holds_every_class(censused, row):
    """Per row, over the chosen subframes of the bases it runs: every class at least twice, and exactly as often as counted when the cases were chosen.
    TOP (a caller in bin 1023 inside the budget: the `bin + 1 < 1024` arm) and SECT_SPENT are found in no trial (GRANT_SWEEP.md: the searches) and are
    absent by name: in no subframe of any base, chosen or not."""
    r = GC.GROW[row]
    cov = GC.coverage(r)
    print(row, cov)
    need = (set(GC.CLASSES) - {"TOP"}) | ({"SECT_CROSS2", "SECT_W64", "SECT_W65"} if GC.sector_row(r) else set())
    assert need <= set(cov) and all(cov[c] >= 2 for c in need), cov
    assert "SECT_SPENT" not in cov and "TOP" not in cov
    assert cov == COVERAGE[row]
    for _, t, _ in GC.bases_of(r):
        assert not any({"TOP", "SECT_SPENT"} & c for c in GC.classes_of(t).values())
    assert not any(row in rows for rows in GC.LEAVES.values())  # (no base leaves a row's kernel: had one, it would be at most one in eight and never a class's only cover)


def test_bases_hold_as_many_bin_form_subframes_as_counted(censused):
    for (tag, rng), (t, _) in GC.distinct_bases().items():
        if "nPreamble65" not in tag:
            assert len(GC.bin_form(t)) == BIN_FORM[(tag.rsplit("_v", 1)[0], t[1])][1 - rng], (tag, rng)


def test_pins_are_what_choose_kernel_predicts():
    """Every (row, base): the cluster size cluster_for picks gives the row's kernel by predict_pin, the next smaller one does not where the row's own size was
    raised; the table of GRANT_SWEEP.md."""
    sizes = {}
    for r in GC.GRANT_ROWS:
        for tag, t, _ in GC.bases_of(r):
            s = GC.sized(r, t[2], t[3])
            assert s is not None, (r["name"], tag)
            got = GC.predict_pin(s["opts"], r["rng"], t[2], t[3])
            want = dict(rec_mode=4, cluster_size=1) if t[3].get("sector_grants") and not r["opts"].get("legacy") else dict(rec_mode=s["pin"].get("rec_mode"), cluster_size=s["pin"]["cluster_size"])
            assert got == want, (r["name"], tag, got, want)
            g, g0 = s["pin"]["cluster_size"], r["pin"]["cluster_size"]
            if g > g0:
                assert GC.predict_pin(dict(r["opts"], cluster=g // 2), r["rng"], t[2], t[3])["rec_mode"] != r["pin"]["rec_mode"]
            sizes.setdefault(r["name"], {})[t[2]] = g
    assert sizes["lcluster16_philox"] == {16384: 16, 16385: 16, 16000: 16, 48000: 16}
    assert sizes["lcluster4_philox"] == {16384: 8, 16385: 8, 16000: 8, 48000: 16}  # (4 032 slots and more on four workgroups, against 3 136)
    assert sizes["lcluster4_glibc"] == {16384: 4, 16385: 8, 16000: 4, 48000: 16}
    assert sizes["cluster4_lds_philox"] == {16384: 8, 16385: 8, 16000: 8, 48000: 16}
    assert sizes["cluster4_global_philox"] == {16384: 4, 16385: 4, 16000: 4, 48000: 4}
    assert GC.ROWS_LEFT_OUT == {} and [r["name"] for r in GC.GRANT_ROWS] == [r["name"] for r in CC.CUT_ROWS if r["program"] == "beta"]
    # predict_pin against pins the kernel-limit table holds for the same engine options (kernel_limits.py, measured there)
    assert GC.predict_pin(dict(cluster=16), 1, 3136 * 16, {}) == dict(rec_mode=3, cluster_size=16) and GC.predict_pin(dict(cluster=16), 1, 3136 * 16 + 64, {})["rec_mode"] == 2
    assert GC.predict_pin(dict(cluster=16), 1, 3712 * 16 + 64, {})["rec_mode"] == 0 and GC.predict_pin(dict(cluster=16), 0, 4096 * 16 + 64, {})["rec_mode"] == 0
    assert GC.predict_pin(dict(cluster=1), 0, 3000, dict(nPreamble=65)) == dict(rec_mode=1, cluster_size=1) and GC.predict_pin(dict(cluster=1), 1, 3000, dict(nPreamble=65))["rec_mode"] == 0


def test_lds_figures_are_the_library_s_own(pkg):
    """predict_pin's LDS sizes against the library's own size functions (host code: no GPU), at every slot count a row of the sweep has and around the
    limits: a changed LDS layout fails here, not only at the pin check on the GPU."""
    import ctypes as C
    L = C.CDLL(pkg.LIB_PATH)
    lean, gen = L._ZN5prach25lcluster_kernel_lds_bytesEibi, L._ZN5prach24cluster_kernel_lds_bytesEibi
    for f in (lean, gen):
        f.restype, f.argtypes = C.c_size_t, [C.c_int, C.c_bool, C.c_int]
    sizes = sorted({n for _, n, _, _ in GC.BASES + GC.SECTOR_BASES})
    for n in sizes:
        groups = (n + 63) // 64
        for g in (2, 4, 8, 16, 32):
            ls = (groups + g - 1) // g * 64
            assert lean(ls, False, 0) == GC.lean_bytes(ls, False, 0) and lean(ls, True, groups) == GC.lean_bytes(ls, True, groups), (n, g)
            assert gen(16, False, ls) == gen(65, False, ls) == GC.general_bytes(ls), (n, g)
    for ls in (64, 3136, 3200, 3712, 3776, 4096):
        assert lean(ls, False, 0) == GC.lean_bytes(ls, False, 0) and gen(54, False, ls) == GC.general_bytes(ls) and lean(ls, True, 4096) == GC.lean_bytes(ls, True, 4096)
    assert GC.LDS_LIMIT == 160 * 1024 and GC.LQCAP == 4096  # (prach_device.h: CLUSTER_LDS_LIMIT, CLUSTER_LQCAP)


def test_every_kernel_with_a_grant_selection_is_run():
    """Every Beta.c / WithNOMA simulation kernel of the built library holds a copy of the selection; each is run by a row of the sweep or named as left out."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "5g-nr-randomaccess_amd", "csrc"), "lib", "ARCH=gfx950"], stdout=subprocess.DEVNULL)
    spec = importlib.util.spec_from_file_location("isa_bitop3", os.path.join(ROOT, "scripts", "isa_bitop3.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    # (only the NAMES of the library's kernel symbols are used, as tests/test_cut_cases_cpu.py does: nothing here looks at a kernel's instructions)
    symbols = {s for s in isa.inventory(isa.SHIPPED) if s.split("<")[0] in ("batch_kernel", "lcluster_kernel", "cluster_kernel", "trial_kernel")}
    assert symbols == set(GC.SELECTION_KERNELS)
    run = {k for r in GC.GRANT_ROWS for k in r["kernels"]}
    assert symbols <= run | set(GC.SYMBOLS_LEFT_OUT) and all(GC.SYMBOLS_LEFT_OUT.values())
    assert all(GC.ROWS_LEFT_OUT[n] and set(CC.ROW[n]["kernels"]) <= run for n in GC.ROWS_LEFT_OUT)  # (a row left out leaves no kernel out)
    # the per-sector form: the batch kernel in all three instantiations, trial_kernel in both
    sect = {k for r in GC.GRANT_ROWS if GC.sector_row(r) for k in r["kernels"]}
    assert sect == {s for s in symbols if s.startswith(("batch_kernel", "trial_kernel"))}


def test_earlier_cases_never_chose_the_bin_form(censused):
    """What the suite held before: no case that is pinned to a kernel or stopped at consecutive subframes enters the bin form, but for default_16000
    (WithNOMA, 17 / 27 subframes of one trial); test_gpu_equals_oracle does, on whichever kernel the engine picks."""
    got, most = {}, 0
    for name, t in _existing_trials():
        got.setdefault(name, {})[(t[1], t[4])] = len(GC.bin_form(t))
        if name != "matrix:default_16000":
            most = max([most] + [ns for _, ns, *_ in GC.census(t)["sub"]])
    assert got == EXISTING and most == EXISTING_MOST
    for (v, n), t in _unpinned_trials():
        assert len(GC.bin_form(t)) == UNPINNED[(v, n)][1 - t[4]], (v, n, t[4])
