"""The host-side table of the grouped reductions (csrc/prach_grouped.h, GROUPED in csrc/prach_host.c) over all eight kinds, without a device: the rows
against include/prach.h, the one merge against numpy, the one refusal sequence of the run entry point in its order, and a sanitised stand-alone run of the
generic shape, merge and CSV functions (tests/tools/grouped_host_check.c).  Shapes: the smallest that can still go wrong — bins 1 and 3, ngroups 1 and 2,
sojourn 2 x 3 and 3 x 2, census axes of 1 and 2 bins."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ERR_ARG, ERR_UNSUPPORTED = -1, -2
CAP = 1 << 27  # words of device buffer a call may ask for (include/prach.h)
KINDS = ("dist", "timeline", "sojourn", "trace", "xtab", "noma_census", "noma_trace", "noma_timeline")  # in the order of PRACH_G_*
# the table of the issue: u64 counters, i64 maxima, the guard counter, the trials a kind takes (0 any, 1 not NOMA.c, 2 NOMA.c with Philox)
TABLE = {"dist": (6, 1, "success", 0), "timeline": (9, 1, "success", 1), "sojourn": (8, 1, "success", 1), "trace": (7, 1, "subframes", 1),
         "xtab": (10, 2, "binned", 1), "noma_census": (11, 2, "binned", 2), "noma_trace": (9, 1, "slots", 2), "noma_timeline": (12, 1, "served", 2)}


class Row(C.Structure):  # prach_grouped_row
    _fields_ = [("spec_bytes", C.c_size_t), ("group_bytes", C.c_size_t), ("counters", C.c_int), ("maxima", C.c_int), ("guard", C.c_int), ("shape", C.c_void_p),
                ("ngroups_at", C.c_size_t), ("reserved_at", C.c_size_t), ("reserved_words", C.c_int), ("trials", C.c_int), ("format", C.c_void_p)]


def classes(pkg):
    return dict(zip(KINDS, (pkg.Dist, pkg.Timeline, pkg.Sojourn, pkg.Trace, pkg.Xtab, pkg.NomaCensus, pkg.NomaTrace, pkg.NomaTimeline)))


def make(pkg, kind, ngroups, variant):
    """An instance of the kind at one of the two small shapes."""
    bins = 3 if variant else 1
    if kind == "dist":
        return pkg.Dist(ngroups, bins, 2)
    if kind == "sojourn":
        return pkg.Sojourn(ngroups, 3 if variant else 2, 500, 2 if variant else 3, 5)
    if kind == "xtab":
        return pkg.Xtab(ngroups, ("arrival", 500, 2 if variant else 1), ("state", 1, 1 if variant else 2), pkg.XTAB_WHO["arrived"])
    if kind == "noma_census":
        return pkg.NomaCensus(ngroups, ("arrival", 500, 2 if variant else 1), ("sector", 1, 1 if variant else 2), pkg.NOMA_WHO["served"])
    return classes(pkg)[kind](ngroups, bins, 5)


def row_of(pkg, kind):
    L = pkg.lib()
    L.prach_internal_grouped_row.restype = C.POINTER(Row)
    L.prach_internal_grouped_row.argtypes = [C.c_int]
    return L.prach_internal_grouped_row(KINDS.index(kind)).contents


@pytest.fixture(scope="module")
def header_sizes(tmp_path_factory):
    """sizeof of every spec and group struct, from a program compiled against include/prach.h"""
    d = tmp_path_factory.mktemp("grouped_sizes")
    types = ["prach_dist_spec", "prach_dist", "prach_timeline_spec", "prach_timeline", "prach_sojourn_spec", "prach_sojourn", "prach_trace_spec", "prach_trace",
             "prach_xtab_spec", "prach_xtab", "prach_xtab_spec", "prach_noma_census", "prach_noma_trace_spec", "prach_noma_trace", "prach_noma_timeline_spec", "prach_noma_timeline"]
    (d / "sz.c").write_text('#include "prach.h"\n#include <stdio.h>\nint main(){' + "".join(f'printf("%zu\\n", sizeof({t}));' for t in types) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(d / "sz.c"), "-o", str(d / "sz")])
    sizes = list(map(int, subprocess.check_output([str(d / "sz")]).split()))
    return {k: (sizes[2 * i], sizes[2 * i + 1]) for i, k in enumerate(KINDS)}


@pytest.mark.parametrize("kind", KINDS)
def test_table_against_header(pkg, header_sizes, kind):
    r, R = row_of(pkg, kind), classes(pkg)[kind]
    counters, maxima, guard, trials = TABLE[kind]
    assert (r.spec_bytes, r.group_bytes) == header_sizes[kind] == (C.sizeof(R._SPEC), C.sizeof(R._STRUCT))
    assert 8 * (r.counters + r.maxima) == r.group_bytes and (r.counters, r.maxima, r.trials) == (counters, maxima, trials)
    assert R._FIELDS[r.guard] == guard and len(R._FIELDS) == counters + maxima and R._MAXIMA == maxima
    assert r.ngroups_at == getattr(R._SPEC, "ngroups").offset and r.reserved_at == getattr(R._SPEC, "reserved").offset
    assert r.reserved_words == getattr(R._SPEC, "reserved").size // 4
    assert not pkg.lib().prach_internal_grouped_row(len(KINDS))  # (NULL: no such kind)


def fill(red, rng, empty):
    """Random counters and arrays; an EMPTY group has a zero guard counter (zero counters and arrays) and garbage in its maxima."""
    for a in red._arrays():
        a[...] = 0 if empty else rng.integers(0, 1 << 40, size=a.shape, dtype=np.uint64)
    nmax = red._MAXIMA
    for f in red._FIELDS[:-nmax]:
        red._scalar(f)[:] = 0 if empty else rng.integers(1, 1 << 40, size=red.ngroups)
    for f in red._FIELDS[-nmax:]:
        red._scalar(f)[:] = rng.integers(0, 1 << 40, size=red.ngroups)
    return red


def reference_merge(into, frm, g, og, guard):
    """The merge in numpy: (scalars, arrays) of group g of `into` after group og of `frm` was added."""
    nmax = into._MAXIMA
    sc = {f: int(into._scalar(f)[g]) + int(frm._scalar(f)[og]) for f in into._FIELDS[:-nmax]}
    for f in into._FIELDS[-nmax:]:
        a = int(into._scalar(f)[g]) if into._scalar(guard)[g] else -1
        b = int(frm._scalar(f)[og]) if frm._scalar(guard)[og] else -1
        sc[f] = max(a, b)
    return sc, [x[g] + y[og] for x, y in zip(into._arrays(), frm._arrays())]


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("ngroups", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_merge_against_numpy(pkg, kind, ngroups, variant):
    L, guard = pkg.lib(), TABLE[kind][2]
    rng = np.random.default_rng(KINDS.index(kind) * 16 + ngroups * 2 + variant)
    for into_empty in (False, True):
        for from_empty in (False, True):
            for public in (False, True):
                a, b = fill(make(pkg, kind, ngroups, variant), rng, into_empty), fill(make(pkg, kind, ngroups, variant), rng, from_empty)
                g, og = ngroups - 1, 0
                want_sc, want_arr = reference_merge(a, b, g, og, guard)
                b_before = [x.copy() for x in b._arrays()] + [b._scalar(f).copy() for f in b._FIELDS]
                others = [x[:g].copy() for x in a._arrays()]
                if public:  # the public function, called as the header declares it
                    sp, da, db = a.spec(), a._group(g), b._group(og)
                    getattr(L, f"prach_{kind}_merge")(C.byref(sp), C.byref(da), *a._cargs(g), C.byref(db), *b._cargs(og))
                    got_sc = {f: getattr(da, f) for f in a._FIELDS}
                else:
                    a.merge_group(g, b, og)
                    got_sc = {f: int(a._scalar(f)[g]) for f in a._FIELDS}
                assert got_sc == want_sc, (kind, into_empty, from_empty, public)
                if into_empty and from_empty:
                    assert all(got_sc[f] == -1 for f in a._FIELDS[-a._MAXIMA:])
                elif into_empty:
                    assert all(got_sc[f] == int(b._scalar(f)[og]) for f in a._FIELDS[-a._MAXIMA:])
                for x, w in zip(a._arrays(), want_arr):
                    assert np.array_equal(x[g], w)
                assert all(np.array_equal(x[:g], o) for x, o in zip(a._arrays(), others))  # the other groups are not touched
                assert all(np.array_equal(x, y) for x, y in zip([*b._arrays()] + [b._scalar(f) for f in b._FIELDS], b_before))  # `from` is only read


def at_the_cap(pkg, kind):
    """(instance with the largest ngroups whose request is at most 2^27 words, words per group): exactly 2^27 words where the words of a group divide it
    (dist at 256 delay bins, sojourn 2 x 2, trace, xtab and the census at 1 x 1 bins), otherwise the last request below (timeline: 5 words, the NOMA pair: 36)."""
    R = classes(pkg)[kind]
    per = {"dist": 512, "timeline": 5, "sojourn": 8, "trace": 4, "xtab": 4, "noma_census": 4, "noma_trace": 36, "noma_timeline": 36}[kind]
    ng = CAP // per
    red = {"dist": lambda: R(1, 256, 1), "sojourn": lambda: R(1, 2, 500, 2, 5), "xtab": lambda: R(1, ("arrival", 500, 1), ("state", 1, 1)),
           "noma_census": lambda: R(1, ("arrival", 500, 1), ("sector", 1, 1))}.get(kind, lambda: R(1, 1, 5))()
    assert sum(int(np.prod(a.shape[1:])) for a in red._arrays()) == per
    red.ngroups = ng  # (only the spec carries it: the arrays stay one group long, no call here gets as far as reading them)
    return red, per


def run(pkg, red, cfgs, group):
    """The kind's run entry point without an engine: the status."""
    n = len(cfgs)
    sp, gg = red.spec(), (red._STRUCT * 1)()
    gp = None if group is None else (C.c_int32 * n)(*group)
    return getattr(pkg.lib(), f"prach_run_trials_{red._KIND}")(None, (pkg.PrachCfg * n)(*cfgs), n, (pkg.PrachResult * n)(), None, C.byref(sp), gp, gg, *red._ptrs(red._RUN))


@pytest.mark.parametrize("kind", KINDS)
def test_refusal_order_without_an_engine(pkg, kind):
    trials = TABLE[kind][3]
    noma = pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX)
    beta = pkg.make_cfg(100, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX)
    right, wrong = (noma, beta) if trials == 2 else (beta, noma)
    red, per = at_the_cap(pkg, kind)
    ng = red.ngroups
    assert ng * per <= CAP < (ng + 1) * per and (ng * per == CAP) == (kind not in ("timeline", "noma_trace", "noma_timeline"))
    assert run(pkg, red, [right], [ng - 1]) == ERR_ARG  # at the cap: accepted as far as the missing engine
    red.ngroups = ng + 1
    assert run(pkg, red, [right], [ng]) == ERR_UNSUPPORTED  # one word-row above it
    assert run(pkg, red, [right], [ng + 1]) == ERR_ARG and run(pkg, red, [right], [-1]) == ERR_ARG  # a bad group id in an oversized request
    assert run(pkg, red, [right, right], None) == ERR_ARG  # ... and no group table with ngroups != n
    red.ngroups = 2
    assert run(pkg, red, [wrong, right], [0, 2]) == ERR_ARG  # a trial of the wrong program with a bad group id
    assert run(pkg, red, [right, wrong], [0, 1]) == (ERR_ARG if trials == 0 else ERR_UNSUPPORTED)  # the wrong program alone (dist takes every program)
    if trials == 2:  # NOMA.c in the reference's own stream is not wired to the menu's device calls
        assert run(pkg, red, [pkg.make_cfg(100, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_GLIBC), right], [0, 1]) == ERR_UNSUPPORTED
    red.ngroups = ng + 1
    assert run(pkg, red, [wrong], [0]) == ERR_UNSUPPORTED  # wrong program and oversized: unsupported either way
    red.ngroups = 0
    assert run(pkg, red, [right], [0]) == ERR_ARG
    red.ngroups = 1
    assert run(pkg, red, [right], [0]) == ERR_ARG  # everything right: the missing engine


def test_sanitised_stand_alone_run(tmp_path):
    """tests/tools/grouped_host_check.c with csrc/prach_host.c under AddressSanitizer and UBSan, as a program of its own on the CPU: exit status 0."""
    cc = shutil.which("gcc") or shutil.which("cc")
    exe = tmp_path / "grouped_host_check"
    src = [os.path.join(ROOT, "tests", "tools", "grouped_host_check.c"), os.path.join(ROOT, "5g-nr-randomaccess_amd", "csrc", "prach_host.c")]
    # (the sanitizer's runtime is linked into the program itself: nothing has to be loaded in front of it)
    subprocess.check_call([cc, "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", *src, "-o", str(exe),
                           "-lm", "-lpthread"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "8 kinds ok" in p.stdout
