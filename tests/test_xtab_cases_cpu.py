"""The synthetic cases of prach::xtab_kernel without a GPU: the generator is deterministic and reaches the states it is there for, the numpy reference equals
the host definition wherever a case's schedules are the product's own, and tests/tools/gpu_xtab_harness.hip compiles for gfx950 and carries the constants
the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import reduce_cases as R  # noqa: E402
import xtab_cases as XC  # noqa: E402
import xtab_ref as X  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return XC.cases(pkg)


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases, tmp_path):
    again = XC.cases(pkg)
    assert tuple(c.name for c in cases) == XC.CASE_NAMES
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and x.E == y.E for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    assert {c.spec[2] for c in cases} == {1, 2, 3, 4, 5, 6, 7}  # every who
    assert sorted({j.nue for j in by["real_census_who_all"].jobs}) == [1, 63, 64, 65, 8191, 8192, 8193, 16385]
    ref = by["real_census_who_all"].reference()
    assert (ref.cells.sum(axis=(0, 1))[1:7] > 0).all() and (ref.scalars["undefined"] == ref.scalars["idle"]).all()  # every STATE, class 6 too; an idle UE has no ARRIVAL
    ref = by["real_one_by_one_idle"].reference()
    assert int(ref.cells[0, 0, 0]) == int(ref.scalars["idle"][0]) == int(ref.cells.sum()) > 0
    ref = by["real_ages_unserved"].reference()
    assert int(ref.scalars["undefined"].sum()) > 0 and int(ref.cells[:, :, 2002].sum()) > 0  # an E below an arrival: no AGE; Uniform arrivals: ages past the last bin
    for name in ("real_window_exact_served", "real_window_plus_one_arrived"):
        c = by[name]
        assert (c.spec[0][2] + 1) * (c.spec[1][2] + 1) == XC.WINDOW_WORDS + (name != "real_window_exact_served")
        ref = c.reference()
        assert int(ref.scalars["undefined"].sum()) > 0 and int(ref.cells[:, -1].sum()) > 0 and int(ref.cells[:, :, -1].sum()) > 0  # negative timers; both overflow bins
    ref = by["real_sojourn_completion_idle_unserved"].reference()
    assert int(ref.scalars["binned"].sum()) == 0 and (ref.scalars["undefined"] == ref.scalars["selected"]).all() and not ref.cells.any()
    assert any(((j.logs[:, R.FLAG] == 1) & (j.logs[:, R.ACTIVE] != -1) & (j.logs[:, R.TXTIME] + 6 < R.arrival_times(j.nue, j.sched, j.access_time))).any()
               for j in by["real_ptc_failcount_idle_served"].jobs)  # a served UE with c < a
    ref = by["bin_edges_and_overflows"].reference()
    assert (ref.cells[0][[0, 1, 2, 8, 9]] > 0).all() and int(ref.cells[0, 3:8].sum()) == 0  # each bin's last and first value, the overflow of each axis and of both at once
    assert int(ref.scalars["row_max"][0]) == int(ref.scalars["col_max"][0]) == 2 ** 31 - 1
    ref = by["all_lanes_one_cell"].reference()
    assert int(ref.cells[0, 2, 3]) == 2 * XC.TILE == int(ref.cells.sum())
    c = by["tiles_without_a_selected_ue"]
    assert all((X.classes(j.logs[XC.TILE:2 * XC.TILE]) == (X.IDLE, X.SERVED)[g]).all() for g, j in enumerate(c.jobs)) and int(c.reference().scalars["binned"][1]) > 0
    assert not (X.classes(c.jobs[1].logs[:XC.TILE]) & X.SERVED).any()
    c = by["long_schedule_and_short_runs"]
    j = c.jobs[0]
    at = R.arrival_times(j.nue, j.sched, 1)
    assert int(at[XC.TILE - 1] - at[0]) > XC.CONSTANTS["XT_SCHED_CAP"] and [x.E for x in c.jobs] == [int(at[-1]) - 1, int(at[-1]), 6000, 0]
    ref = c.reference()
    assert ref.scalars["undefined"].tolist()[1:3] == [0, 0] and 0 < int(ref.scalars["undefined"][0]) < 8 and int(ref.scalars["undefined"][3]) > XC.TILE
    p = str(tmp_path / "case.bin")
    XC.write_case(by["all_lanes_one_cell"], p)
    assert os.path.getsize(p) == 4 * (16 + 8 + 16 * 2 * XC.TILE + 2)


def test_reference_equals_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert XC.same(host, ref) is None, (c.name, XC.same(host, ref))
        seen += 1
    assert seen == 7


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = XC.build_harness(tmp_path)
    assert R.harness_constants(exe) == XC.CONSTANTS
    assert XC.CONSTANTS["XT_WINDOW_WORDS"] == pkg.xtab_window_words() and XC.CONSTANTS["TL_TILE"] == pkg.xtab_tile_ues()
