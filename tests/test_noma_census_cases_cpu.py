"""The synthetic cases of prach::noma_census_kernel and prach::noma_columns_kernel without a GPU: the generator is deterministic and reaches the states it
is there for, the numpy restatement equals both host definitions wherever a case's schedules are the product's own, and
tests/tools/gpu_noma_census_harness.hip compiles for gfx950 and carries the constants the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import noma_census_cases as NC  # noqa: E402
import noma_census_ref as N  # noqa: E402
import reduce_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return NC.cases(pkg)


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases, tmp_path):
    again = NC.cases(pkg)
    assert tuple(c.name for c in cases) == NC.CASE_NAMES
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and x.E == y.E for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    c = by["real_census_who_all"]
    assert sorted(j.nue for j in c.jobs) == [1, 63, 64, 65, 8191, 8192, 8193, 16385]
    ref = c.reference()
    assert (ref["cells"].sum(axis=(0, 1))[1:9] > 0).all() and (ref["scalars"]["undefined"] == ref["scalars"]["idle"]).all()  # every STATE, 8 too; an idle UE has no ARRIVAL
    logs = np.concatenate([j.logs for j in c.jobs])
    fail = logs[:, N.W_FAIL].astype(np.int64)
    assert ((fail & 0xffff != 0) & (fail >> 16 > 0)).any() and (fail < 0).any() and (logs[:, N.W_TIMER] < 0).any() and (logs[:, N.W_TXTIME] < 0).any()  # both halves set; negative words
    assert (logs[:, N.W_SECTOR] < -1).any() and (logs[:, N.W_SECTOR] > 5).any() and ((logs[:, N.W_SECTOR] == -1) & (logs[:, N.W_RA] == 1)).any()
    for name, cells in (("real_copies_below", NC.COPY_CELLS - 1), ("real_copies_exact", NC.COPY_CELLS), ("real_copies_above", NC.COPY_CELLS + 1),
                        ("real_window_below", NC.WINDOW_WORDS - 1), ("real_window_exact", NC.WINDOW_WORDS), ("real_window_above", NC.WINDOW_WORDS + 1)):
        c = by[name]
        assert (c.spec[0][2] + 1) * (c.spec[1][2] + 1) == cells
        ref = c.reference()
        assert int(ref["scalars"]["binned"].sum()) > 0 and int(ref["cells"][:, -1].sum()) + int(ref["cells"][:, :, -1].sum()) > 0, name  # an overflow bin is hit
    assert {c.spec[2] for c in cases} >= {N.ALL, N.IDLE, N.SERVED, N.SERVED | N.PENDING, N.DROPPED | N.PENDING}
    ref = by["real_one_by_one_idle"].reference()
    assert int(ref["cells"][0, 0, 0]) == int(ref["scalars"]["idle"][0]) == int(ref["cells"].sum()) > 0
    ref = by["bin_edges_and_overflows"].reference()
    assert (ref["cells"][0][[0, 1, 2, 8, 9]].sum(axis=1) > 0).all() and int(ref["cells"][0, 3:8].sum()) == 0  # each bin's last and first value, the overflow of each axis
    assert int(ref["cells"][0, 9, 4]) > 0 and int(ref["scalars"]["row_max"][0]) == 0x7fff and int(ref["scalars"]["col_max"][0]) == 2 ** 31 - 1  # ... and of both at once
    c = by["all_lanes_one_cell"]
    ref = c.reference()
    assert c.jobs[0].nue % NC.TILE == 1 and int(ref["cells"][0, 5, 3]) == 2 * NC.TILE + 1 == int(ref["cells"].sum())  # a tile of one UE; everybody stranded
    c = by["tiles_without_a_selected_ue"]
    assert all((N.classes(j.logs[NC.TILE:2 * NC.TILE]) == (N.IDLE, N.SERVED)[g]).all() for g, j in enumerate(c.jobs)) and int(c.reference()["scalars"]["binned"][1]) > 0
    assert not (N.classes(c.jobs[1].logs[:NC.TILE]) & N.SERVED).any()
    c = by["long_schedule_and_short_runs"]
    j = c.jobs[0]
    at = R.arrival_times(j.nue, j.sched, 1)
    assert int(at[NC.TILE - 1] - at[0]) > NC.CONSTANTS["TILE_SCHED_CAP"] and [x.E for x in c.jobs] == [int(at[-1]) - 1, int(at[-1]), 6000, 0]
    c = by["raw_words_of_every_quarter"]  # no menu field of these columns reads quarter 0 or 1; a raw word of every quarter stands next to them
    assert c.columns != NC.COLUMN_FIELDS and {(f - N.RAW) >> 2 for f in c.columns if f >= N.RAW} == {0, 1, 2, 3}
    assert {f for f in c.columns if f < N.RAW} == {N.PTC, N.ARRIVAL} and not {c.spec[0][0], c.spec[1][0]} & {N.SOJOURN, N.COMPLETION, N.TIMER, N.STATE, N.LOST, N.PREAMBLE}
    p = str(tmp_path / "case.bin")
    NC.write_case(by["all_lanes_one_cell"], p)
    assert os.path.getsize(p) == 4 * (32 + 8 + 16 * (2 * NC.TILE + 1) + 2)


def test_references_equal_the_host_definitions(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert NC.same(host, ref) is None, (c.name, NC.same(host, ref))
        (rd, rc), (hd, hc) = c.reference_columns(), c.host_columns(pkg)
        assert np.array_equal(rd, hd) and np.array_equal(rc, hc), c.name
        seen += 1
    assert seen == 9


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = NC.build_harness(tmp_path)
    assert R.harness_constants(exe) == NC.CONSTANTS
    assert NC.CONSTANTS["XT_WINDOW_WORDS"] == pkg.xtab_window_words() and NC.CONSTANTS["TL_TILE"] == pkg.noma_census_tile_ues()
    assert NC.CONSTANTS["NC_COPY_WORDS"] == 4 * NC.COPY_CELLS
