"""The synthetic cases of prach::summary_kernel without a GPU: the generator is deterministic and reaches the states it is there for, the numpy restatement
of the kernel's row equals the host definition wherever a case's schedules are the product's own, and tests/tools/gpu_summary_harness.hip compiles for
gfx950 and carries the constants the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import reduce_cases as R  # noqa: E402
import summary_cases as SC  # noqa: E402

ARRIVED, SUCCESS, RERR, MAXV, Q = 0, 1, 3, 9, 12  # words of a row


@pytest.fixture(scope="module")
def cases(pkg):
    return SC.cases(pkg)


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases, tmp_path):
    again = SC.cases(pkg)
    assert tuple(c.name for c in cases) == SC.CASE_NAMES
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    ref = {n: by[n].reference() for n in SC.CASE_NAMES}
    assert ref["one_successful_ue"][:, SUCCESS].tolist() == [1, 1] and ref["one_successful_ue"][0, Q:Q + 3].tolist() == [4321] * 3
    r = ref["all_on_one_value"][0]
    assert r[SUCCESS] == 3000 and r[Q:Q + 4].tolist() == [777] * 4 and r[Q + 16:Q + 20].tolist() == [3] * 4
    assert ref["split_63_64"][0, Q:Q + 2].tolist() == [63, 64] and ref["split_63_64"][0, Q + 16:Q + 18].tolist() == [63, 64]
    r = ref["eight_levels_eight_coarse_bins"][0]
    assert len(set((r[Q:Q + 8] >> 6).tolist())) == 8 and len(set((r[Q + 8:Q + 16] >> 6).tolist())) == 8
    r = ref["eight_levels_one_coarse_bin"][0]
    assert set((r[Q:Q + 8] >> 6).tolist()) == {100} and set((r[Q + 8:Q + 16] >> 6).tolist()) == {1023} and set((r[Q + 16:Q + 24] >> 6).tolist()) == {0}
    assert len(set(r[Q:Q + 8].tolist())) >= 6
    r = ref["values_0_60005_65535"]
    assert set(r[0, Q:Q + 6].tolist()) == {0, 60005, 65535} and r[1, MAXV:MAXV + 3].tolist() == [65535, 0, 65535] and not r[:, RERR:RERR + 3].any()
    r = ref["one_value_65536"]
    assert r[:, RERR:RERR + 3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for q in range(3):  # the largest rank lies beyond the values in range; the maximum and the sum still hold the value
        assert r[q, Q + 8 * q + 2] == -1 and r[q, Q + 8 * q] >= 0 and r[q, MAXV + q] == 65536 and (r[q, Q + 8 * ((q + 1) % 3):Q + 8 * ((q + 1) % 3) + 3] >= 0).all()
    assert sorted({j.nue for j in by["sizes_real_schedules"].jobs}) == [1, 63, 65, 1023, 1025, 8193]
    assert any(len(j.sched) > SC.SCHED_CAP for j in by["sizes_real_schedules"].jobs) and not ref["sizes_real_schedules"][:, RERR:RERR + 3].any()
    r = ref["nobody_arrived_nobody_successful_no_slot"]
    assert r[0, :3].tolist() == [0, 0, 0] and r[1, :3].tolist() == [300, 0, 0] and (r[:2, MAXV:] == -1).all() and r[2, SUCCESS] > 100
    j = by["orders_differ"].jobs[0]
    assert np.argmax(j.logs[:, R.TXTIME]) != np.argmax(j.logs[:, R.TIMER]) != np.argmax(j.logs[:, SC.PTC])
    assert [len(j.sched) for j in by["schedule_around_the_staging_limit"].jobs] == [SC.SCHED_CAP, SC.SCHED_CAP + 1]
    assert len(by["jobs_1500"].jobs) == 1500 and (ref["jobs_1500"][:, SUCCESS] == 0).any() and not ref["jobs_1500"][:, RERR:RERR + 3].any()
    p = str(tmp_path / "case.bin")
    SC.write_case(by["split_63_64"], p)
    assert os.path.getsize(p) == 4 * (16 + 8 + sum(16 * j.nue + len(j.sched) for j in by["split_63_64"].jobs))


def test_reference_equals_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert SC.same(host, ref) is None, (c.name, SC.same(host, ref))
        seen += 1
    assert seen == 1


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = SC.build_harness(tmp_path)
    assert R.harness_constants(exe) == SC.CONSTANTS
    assert SC.CONSTANTS["SM_MAX_VALUE"] == pkg.summary_max_value() == SC.MAX_VALUE and 8 * SC.WORDS >= 12 * 8 + 3 * 8 * 8
