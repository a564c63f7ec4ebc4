"""The synthetic cases of prach::sojourn_kernel without a GPU: the generator is deterministic and reaches the states it is there for, the numpy reference
equals the host definition wherever a case's schedules are the product's own, and tests/tools/gpu_sojourn_harness.hip compiles for gfx950 and carries the
constants the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import reduce_cases as R  # noqa: E402
import sojourn_cases as SC  # noqa: E402
import sojourn_ref as S  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return SC.cases(pkg)


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases, tmp_path):
    again = SC.cases(pkg)
    assert tuple(c.name for c in cases) == SC.CASE_NAMES and 10 <= len(cases) <= 14
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    ref = by["one_cell_in_window"].reference()
    assert sorted(int(v) for v in ref.hist.max(axis=(1, 2))) == [R.TILE, R.TILE, R.TILE, R.TILE + 3, R.TILE + 3, R.TILE + 3]  # whole trials in ONE cell
    assert ref.scalars["sojourn_max"].tolist() == [0, 0, R.MAX_SOJOURN, R.MAX_SOJOURN, R.MAX_SOJOURN + 1, R.MAX_SOJOURN + 1]
    ref = by["one_cell_behind_window"].reference()
    assert int(ref.row_arrived[0, 0]) == 1 and int(ref.row_arrived[0, 3]) == R.TILE - 1  # the tile's first UE anchors the window three rows in front of the rest
    sizes = {j.nue % 4 for j in by["real_schedules_1x1_1x1"].jobs}
    assert sizes == {0, 1, 2, 3}
    assert any((j.logs[R.TILE:2 * R.TILE, R.ACTIVE] == -1).all() for j in by["real_schedules_21x500_2002x5"].jobs if j.nue > 2 * R.TILE)  # a tile nobody activated
    ref = by["real_schedules_behind_last_row"].reference()
    assert int(ref.scalars["arrival_overflow"].sum()) > 0 and int(ref.row_delay_overflow.sum()) > 0
    c = by["real_schedules_behind_last_row"]
    assert c.spec[2] * c.spec[3] <= R.MAX_SOJOURN < (c.spec[2] + 1) * c.spec[3]  # a sojourn in the FIRST bin of the overflow: `>` for `>=` would miss it
    assert any(((j.logs[:, R.FLAG] == 1) & (j.logs[:, R.ACTIVE] != -1) & (j.logs[:, R.TXTIME] + 6 - R.arrival_times(j.nue, j.sched, j.access_time) == R.MAX_SOJOURN)).any() for j in c.jobs)
    ref = by["no_slot_and_idle_tiles"].reference()
    assert int(ref.scalars["arrival_overflow"][0]) > R.TILE // 2  # the UEs no slot activates arrive behind the last row
    assert len(by["jobs_1500_groups_5"].jobs) == 1500
    for name in ("window_edges_row1", "window_edges_row3"):
        c = by[name]
        ref = c.reference()
        rows = np.flatnonzero(ref.row_arrived[0])
        assert rows[0] == 1000 and {1000 + R.WINDOW - 1, 1000 + R.WINDOW, 4095} <= set(rows.tolist()) and int(ref.scalars["arrival_overflow"][0]) > 0
    p = str(tmp_path / "case.bin")
    SC.write_case(by["one_cell_in_window"], p)
    assert os.path.getsize(p) == 4 * (16 + 8 * 6 + sum(16 * j.nue + len(j.sched) for j in by["one_cell_in_window"].jobs))


def test_reference_equals_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert SC.same(host, ref) is None, (c.name, SC.same(host, ref))
        seen += 1
    assert seen == 5


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = SC.build_harness(tmp_path)
    assert R.harness_constants(exe) == SC.CONSTANTS
    assert SC.CONSTANTS["SJ_WINDOW_WORDS"] == pkg.sojourn_window_words() and SC.CONSTANTS["TL_TILE"] == pkg.sojourn_tile_ues()
