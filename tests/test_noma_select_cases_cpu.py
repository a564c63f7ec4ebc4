"""The synthetic cases of prach::noma_summary_kernel and prach::noma_pick_kernel without a GPU: the generator is deterministic and reaches the states it is
there for, the numpy restatement equals both host definitions wherever a case's schedules are the product's own, and
tests/tools/gpu_noma_select_harness.hip compiles for gfx950 and carries the constants the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_census_ref as N  # noqa: E402
import noma_select_cases as SC  # noqa: E402
import noma_select_ref as S  # noqa: E402
import reduce_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return SC.cases(pkg)


@pytest.fixture(scope="module")
def refs(cases):
    return {c.name: c.reference() for c in cases}


def test_generator_is_deterministic(pkg, cases, tmp_path):
    again = SC.cases(pkg)
    assert tuple(c.name for c in cases) == SC.CASE_NAMES
    for a, b in zip(cases, again):
        assert a.spec == b.spec and len(a.jobs) == len(b.jobs)
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and x.E == y.E for x, y in zip(a.jobs, b.jobs))
    p = str(tmp_path / "case.bin")
    c = cases[1]
    SC.write_case(c, p)
    assert os.path.getsize(p) == 4 * (32 + 8 * len(c.jobs) + sum(16 * j.nue + len(j.sched) for j in c.jobs))


def test_summary_cases_reach_their_states(cases, refs):
    by = {c.name: c for c in cases}
    c = by["summary_sizes_eight_levels"]
    assert [j.nue for j in c.jobs] == list(SC.SIZES) and c.spec[0][0] == c.spec[0][2] and len(c.spec[2]) == 8  # the same field twice, eight levels
    logs = np.concatenate([j.logs for j in c.jobs])
    E = c.jobs[-1].E
    assert set(np.unique(N.states(c.jobs[-1].logs, E))) == set(range(9))  # every STATE, 8 too
    fail = logs[:, N.W_FAIL].astype(np.int64)
    assert ((fail & 0xffff != 0) & (fail >> 16 > 0)).any() and ((fail & 0xffff == 0) & (fail >> 16 > 0)).any() and (fail == -2 ** 31).any()
    assert (logs[:, N.W_TIMER] < 0).any() and (logs[:, N.W_TXTIME] < 0).any() and (logs[:, N.W_PTC] < 0).any() and ((logs[:, N.W_SECTOR] == -1) & (logs[:, N.W_RA] == 1)).any()
    rows = refs[c.name]
    assert all(r["q"][0].tolist() == r["q"][2].tolist() and r["n"][0] == r["n"][2] for r in rows) and rows[-1]["n"][1] > 0 and not any(r["range_errors"] for r in rows)

    c = by["summary_values_and_ranks"]
    rows = refs[c.name]
    assert rows[0]["q"][0].tolist() == [0, 65535, 63, 0, 64, 65535, 65535, 65535] and rows[0]["max"][0] == 65535  # ranks 1, 4, 2, 1, 3, 4, 4, 4 of 0, 63, 64, 65 535
    assert rows[1]["q"][0].tolist() == [0] * 8 and rows[2]["q"][0].tolist() == [65535] * 8
    r = rows[5]  # the one 65 536: TIMER's levels are void, PTC's stay
    assert r["range_errors"] == 1 and r["max"][0] == 65536 and r["n"][0] == 1000 and (r["q"][0] == -1).all() and (r["q"][1] >= 0).all() and r["sum"][0] > 65536
    assert rows[6]["q"][0].tolist() == [4242] * 8 and rows[6]["sum"][0] == 777 * 4242
    assert len({int(v) >> 6 for v in rows[7]["q"][0]}) == 1 and len(set(rows[7]["q"][0].tolist())) > 4  # eight levels, one coarse bin, several fine bins
    assert S.rank(1000, 500) == 500 and S.rank(1001, 500) == 501 and rows[8]["q"][0][2] == 499 * 60 and rows[9]["q"][0][2] == 500 * 60
    assert S.rank(1000, 1) == 1 and S.rank(1000, 1000) == 1000 and S.rank(3, 1) == 1

    c = by["summary_undefined_field_and_one"]
    rows = refs[c.name]
    assert all(r["n"][0] == 0 and r["max"][0] == -1 and (r["q"][0] == -1).all() for r in rows)  # SOJOURN of the pending: undefined for every selected UE
    assert any(r["n"][1] == r["selected"] > 0 and r["q"][1][:2].tolist() == [0, 0] and r["max"][1] == 0 for r in rows)  # ONE
    assert any(r["selected"] == 0 and (r["q"] == -1).all() for r in rows)

    c = by["summary_schedules_and_ends"]
    assert sorted({len(j.sched) for j in c.jobs}) == [SC.SCHED_CAP, SC.SCHED_CAP + 1]
    for base in (0, 4):
        at = R.arrival_times(c.jobs[base].nue, c.jobs[base].sched, 1)
        assert [j.E for j in c.jobs[base:base + 4]] == [int(at[-1]) - 1, int(at[-1]), len(c.jobs[base].sched), 0]
    rows = refs[c.name]
    assert rows[3]["n"][0] < 10 and rows[3]["selected"] == 1500 and rows[2]["n"][0] > 1000  # AGE: undefined for the UEs that arrive behind E = 0


def test_pick_cases_reach_their_states(cases, refs):
    by = {c.name: c for c in cases}
    assert {c.spec[3] for c in cases if c.kind == "pick"} >= {1, 4096}
    hdrs = [h for h, _ in refs["pick_index_k1_sizes"]]
    assert all(h["stored"] == 1 == h["matched"] if j.nue == 1 else h["stored"] == 1 < h["matched"] for h, j in zip(hdrs, by["pick_index_k1_sizes"].jobs))

    c = by["pick_index_k4096_four_clauses"]
    assert len(c.spec[0]) == 4
    hdrs = [h for h, _ in refs[c.name]]
    assert [h["matched"] for h in hdrs[-4:]] == [0, 4095, 4096, 4097] and [h["stored"] for h in hdrs[-4:]] == [0, 4095, 4096, 4096]
    # a clause that fails next to an undefined needed value is not counted in `undefined`: such UEs exist, and `undefined` is smaller than their number plus the rest
    j = c.jobs[len(SC.SIZES) - 1]
    sel = (N.classes(j.logs) & c.spec[4]) != 0
    sj, tm = N.values(N.SOJOURN, j.logs, j.sched, j.access_time, j.E), N.values(N.TIMER, j.logs, j.sched, j.access_time, j.E)
    both = sel & (sj < 0) & (tm >= 0) & ((tm < 10) | (tm > 600))
    h = hdrs[len(SC.SIZES) - 1]
    assert both.sum() > 0 and 0 < h["undefined"] <= int((sel & ((sj < 0) | (tm < 0))).sum()) - int(both.sum()) and h["matched"] > 0

    for name, mirror in (("pick_largest_ties", False), ("pick_smallest_ties", True)):
        c = by[name]
        out = refs[name]
        assert c.spec[3] == 64
        for q, (start, left_out) in enumerate((s, l) for s in (50, 490, 1000) for l in (0, 3, 1000)):
            h, rows = out[q]
            assert (h["matched"], h["stored"], h["ties_left_out"], h["threshold"]) == (3000, 64, left_out, 65035 if mirror else 500)
            assert rows[:20, 0].tolist() == list(range(2500, 2520)) and rows[20:64, 0].tolist() == list(range(start, start + 44))  # the ties that are taken: the first 44
        assert any(s <= e - 1 and e < s + 44 for s in (50, 490, 1000) for e in (64, 512, 1024))  # the taken ties straddle each edge once
        assert [(h["matched"], h["stored"]) for h, _ in out[9:12]] == [(63, 63), (64, 64), (65, 64)] and out[9][0]["ties_left_out"] == 0 and out[11][0]["ties_left_out"] == 1
        h, rows = out[12]  # keys 0 and 65 535
        assert h["threshold"] == (0 if mirror else 65535) and h["stored"] == 64 and h["ties_left_out"] > 0
        assert out[13][0]["range_errors"] == 1 and out[13][0]["stored"] == 0 and out[13][0]["matched"] == 600 and not out[13][1].any()
        assert out[14][0]["range_errors"] == 70 == out[14][0]["matched"] and out[14][0]["threshold"] == -1

    c = by["pick_largest_age_schedules_and_ends"]
    out = refs[c.name]
    assert out[3][0]["undefined"] > 100 and out[3][0]["matched"] < 10  # E = 0: AGE is undefined for whoever arrives later
    assert out[2][0]["undefined"] == 0 and out[2][0]["stored"] == out[2][0]["matched"] > 100 and out[2][0]["ties_left_out"] == 0

    c = by["pick_index_idle_rows"]  # three blocks of either shape, idle UEs (arrival -1) among the 300 stored rows of each trial
    assert [j.nue for j in c.jobs] == [1025, 2049] and c.spec[3] == 300
    for j, (h, rows) in zip(c.jobs, refs[c.name]):
        idle = N.classes(j.logs[rows[:, 0]]) == N.IDLE
        assert h["stored"] == 300 and rows[:, 0].tolist() == list(range(300)) and 0 < idle.sum() < 300 and (rows[idle, 16] == -1).all() and (rows[~idle, 16] >= 0).all()


def test_references_equal_the_host_definitions(pkg, cases, refs):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        host = SC.host_rows(c, c.host_definition(pkg))
        assert SC.same(c, host, refs[c.name]) is None, (c.name, SC.same(c, host, refs[c.name]))
        seen += 1
    assert seen == 4


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = SC.build_harness(tmp_path)
    assert R.harness_constants(exe) == SC.CONSTANTS
    assert SC.CONSTANTS["NS_MAX_KEY"] == pkg.summary_max_value() == S.MAX_VALUE and SC.CONSTANTS["NSM_WORDS"] == SC.NSM_WORDS == 22 + 4 * 8
    # two workgroups per CU with the longest staged schedule: 80 KiB each
    assert 4 * (SC.CONSTANTS["NSM_LDS_WORDS"] + SC.SCHED_CAP) <= 80 * 1024 and 4 * (SC.CONSTANTS["NS_LDS_WORDS"] + SC.SCHED_CAP) <= 80 * 1024
