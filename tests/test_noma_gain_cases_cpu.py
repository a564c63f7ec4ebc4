"""The synthetic cases of the two kernels of prach_noma_gain.hip without a GPU: the generator is deterministic and reaches the states it is there for, the numpy
restatement equals the host definition wherever a case's schedules are the product's own, the level cases sit where they are meant to sit against the band,
and tests/tools/gpu_noma_gain_harness.hip compiles for gfx950, accepts every case under --check, refuses malformed files with exit code 3 and carries the
constants the generator assumes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_census_ref as N  # noqa: E402
import noma_gain_cases as GC  # noqa: E402
import noma_gain_ref as G  # noqa: E402

TILE, INT_MIN, INT_MAX = GC.TILE, GC.INT_MIN, GC.INT_MAX


@pytest.fixture(scope="module")
def cases(pkg):
    return GC.cases(pkg)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return GC.build_harness(tmp_path_factory.mktemp("noma_gain_harness"))


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases):
    again = GC.cases(pkg)
    assert tuple(c.name for c in cases) == GC.CASE_NAMES
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and np.array_equal(x.level, y.level) and (x.E, x.group) == (y.E, y.group)
                   for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    refs = {c.name: c.reference() for c in cases}
    assert all(G.identity(r) for r in refs.values())

    c = by["sizes_wild_records"]
    assert sorted(j.nue for j in c.jobs) == [1, TILE - 1, TILE, TILE + 1, 3 * TILE]
    logs = np.concatenate([j.logs for j in c.jobs])
    cls = N.classes(logs)
    arrived, sv = cls != N.IDLE, cls == N.SERVED
    assert set(np.unique(cls)) == {N.SERVED, N.PENDING, N.IDLE, N.DROPPED}
    assert set(np.unique(np.concatenate([N.states(j.logs, j.E) for j in c.jobs]))) == set(range(9))  # every STATE, 8 too
    assert {6, INT_MIN, 7, -2} <= set(logs[arrived, N.W_SECTOR].tolist())
    assert (logs[sv, N.W_TIMER] < 0).any() and (logs[sv, N.W_TXTIME] < 0).any() and (logs[sv, N.W_PTC] < 0).any()  # negative SOJOURN / TIMER / PTC words on served UEs
    r = refs[c.name]["scalars"]
    assert (r["undefined"][:3] > 0).all() and (r["restarted"][:3] > 0).all() and r["below"].sum() > 0 and r["above"].sum() > 0 and (refs[c.name]["series"].sum(axis=(1, 2, 3)) > 0).all()

    for name, bins, width, lo in (("sizes_wild_records", 65, 200, -16200), ("edges_bins2", 2, 7, -50), ("bins1_width_2p20_lo_int_min", 1, 2 ** 20, INT_MIN + 1),
                                  ("bins4096_width1_positive_lo", 4096, 1, 1000), ("lds_limit_bins511", 511, 25, -16200), ("lds_limit_bins512", 512, 25, -16200)):
        c = by[name]
        assert (c.bins, c.width, c.lo) == (bins, width, lo)
        L = np.concatenate([j.level for j in c.jobs]).astype(np.int64)
        hi = lo + bins * width
        want = {lo, hi - 1, lo - 1, hi, INT_MIN} if lo - 1 >= INT_MIN else {lo, hi - 1, hi}
        if lo - 1 < INT_MIN:
            assert lo - 1 == INT_MIN  # one below the lowest lower edge IS "no level"
        assert {v for v in want if INT_MIN <= v <= INT_MAX} <= set(L.tolist()), name
        if bins <= 64:
            assert {lo + b * width for b in range(1, bins)} <= set(L.tolist())  # every inner edge
        arr = refs[name]["series"][G.ARRIVED].sum(axis=(0, 1))
        assert arr[0] > 0 and arr[-1] > 0 and int(refs[name]["scalars"]["above"].sum()) > 0 and (lo - 1 <= INT_MIN or int(refs[name]["scalars"]["below"].sum()) > 0)
    assert GC.LDS_MAX_BINS == 511 and by["bins4096_width1_positive_lo"].lo > 0 and (refs["bins4096_width1_positive_lo"]["scalars"]["level_max"] > 0).all()

    c = by["budget_addends_and_sums_past_2p32"]
    a = c.jobs[0].logs.astype(np.int64)
    M = GC.MAX_ADDEND
    assert {M, M + 1, INT_MAX} <= set(a[:, N.W_PTC].tolist()) and c.jobs[0].nue == 2 * TILE + 3 and TILE * M < 2 ** 32
    r = refs[c.name]
    assert int(r["scalars"]["served"][0]) == c.jobs[0].nue == int(r["series"][G.SERVED].sum()) and int(r["scalars"]["undefined"][0]) == 0
    cells = r["series"][G.PTC_SUM, 0, 3]
    assert (cells > 0).sum() == 2 and cells.max() > 2 ** 32 and int(r["series"][G.SOJOURN_SUM].sum()) == int(r["scalars"]["sojourn_sum"][0]) > 2 ** 31  # a sum past 2^32 in ONE cell
    c = by["jobs_300_groups_3"]
    assert len(c.jobs) == 300 and c.ngroups == 3 and {j.group for j in c.jobs} == {0, 1, 2} and not c.host


def test_references_equal_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert G.same(host, ref) is None, (c.name, G.same(host, ref))
        seen += 1
    assert seen == len(GC.CASE_NAMES) - 1


def test_level_cases_sit_where_they_are_meant_to(pkg):
    cases = GC.level_cases()
    assert tuple(c.name for c in cases) == GC.LEVEL_CASE_NAMES
    c = cases[0]
    edges = c.expected_edges()
    assert c.inside <= edges and not (c.outside & edges) and len(c.inside) >= 20 and len(c.outside) >= 20
    assert sorted(j.nue for j in c.jobs) == [1, 70, TILE + 1] and {k for k, _ in edges} == {0, 1, 2} and len(edges) <= len(c.inside) + 2  # hardly any ordinary value is EDGE
    lv = c.expected_levels()
    assert (lv == G.NO_LEVEL).sum() >= 5 and lv.max() == 40500 and lv.min() == G.NO_LEVEL
    for k, j in enumerate(c.jobs):  # the products really lie inside / outside the band, on both sides of the integer and on it
        p = GC.product_of(j.lgain)
        with np.errstate(invalid="ignore"):
            d = p - np.floor(p)
        ins = [i for q, i in c.inside if q == k and np.isfinite(p[i]) and abs(p[i]) < GC.RANGE]
        outs = [i for q, i in c.outside if q == k]
        assert all(d[i] <= GC.BAND or d[i] >= 1 - GC.BAND for i in ins) and all(GC.BAND < d[i] < 1 - GC.BAND for i in outs)
        if k == 1:
            assert any(0 < d[i] <= GC.BAND for i in ins) and any(d[i] >= 1 - GC.BAND for i in ins) and any(d[i] == 0 for i in ins)
            assert any(GC.BAND < d[i] < 1e-7 for i in outs) and any(1 - 1e-7 < d[i] < 1 - GC.BAND for i in outs)
        assert [pkg.noma_gain_level(float(x)) for x in j.lgain[:200]] == G.level_of(j.lgain[:200]).tolist()
    c = cases[1]
    assert c.cap == 8 and len(c.expected_edges()) == 9 == len(c.inside) and c.expected_edges() == c.inside


def test_harness_checks_every_case_and_refuses_malformed_files(cases, harness, tmp_path):
    good = None
    for c in list(cases) + GC.level_cases():
        p = str(tmp_path / f"{c.name}.bin")
        GC.write_case(c, p)
        assert os.path.getsize(p + ".side") == 12 * sum(j.nue for j in c.jobs)
        H.run(harness, ["--check", p], timeout=60)
        good = good or p
    raw = np.fromfile(good, dtype="<i4")

    def refused(words, name, nbytes=None):
        p = str(tmp_path / f"bad_{name}.bin")
        b = np.ascontiguousarray(words, dtype="<i4").tobytes()
        with open(p, "wb") as f:
            f.write(b if nbytes is None else b[:nbytes])
        r = subprocess.run([harness, "--check", p], capture_output=True, text=True, timeout=60)
        assert r.returncode == 3 and "gpu_noma_gain_harness" in r.stderr, (name, r.returncode, r.stderr)

    def patched(at, v):
        w = raw.copy()
        w[at] = v
        return w

    refused(raw[:-1], "truncated")
    refused(np.append(raw, 0), "trailing")
    refused(raw, "odd_length", nbytes=raw.nbytes - 2)
    refused(patched(0, 1), "magic")
    refused(patched(1, 13), "kind")
    refused(patched(2, 0), "njobs")
    for at, v, name in ((3, 0, "bins0"), (3, 4097, "bins"), (4, 0, "width"), (6, 0, "ngroups0"), (6, 65, "ngroups")):
        refused(patched(at, v), name)
    row = 16  # the first job row: nUE, group, form, accessTime, nslots, E
    for at, v, name in ((row, 0, "nue"), (row + 1, 4, "group"), (row + 1, -1, "group_neg"), (row + 3, 0, "access_time"), (row + 4, 0, "nslots"), (row + 5, -1, "E")):
        refused(patched(at, v), name)
    # a mode, a capacity or a side file out of range is refused before any HIP call
    for args in (["3", good + ".side"], ["2", good + ".side", "-1"], ["2", good + ".side", str(GC.EDGE_CAP + 1)], ["0", good], ["0", str(tmp_path / "none")]):
        r = subprocess.run([harness, good, str(tmp_path / "r"), *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 3, (args, r.returncode, r.stderr)


def test_harness_carries_the_constants(pkg, harness):
    assert H.constants(harness, parse=float) == {k: float(v) for k, v in GC.CONSTANTS.items()}
    assert GC.CONSTANTS["TL_TILE"] == pkg.noma_gain_tile_ues() and GC.CONSTANTS["NG_LDS_MAX_BINS"] == pkg.noma_gain_lds_max_bins()
    assert GC.CONSTANTS["TL_TILE"] * GC.CONSTANTS["NG_MAX_ADDEND"] < 2 ** 32 and GC.BAND == 1e-8
