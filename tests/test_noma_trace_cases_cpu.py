"""tests/tools/noma_trace_cases.py without a GPU: the numpy reference equals the plain loop over the rows that csrc/prach_noma_trace.hip names as its
definition, the generated cases contain what they are there for, every case file passes the harness's own checks, and
tests/tools/gpu_noma_trace_harness.hip compiles for gfx950 and carries the constants the generator places its sizes around."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_trace_cases as N  # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in N.cases()}


def plain_loop(case):
    series = [[[[0] * case.bins for _ in range(6)] for _ in range(case.ngroups)] for _ in range(6)]
    sc = [[0] * N.NSC for _ in range(case.ngroups)]
    for j in case.jobs:
        g = sc[j.group]
        slots = set()
        for r, row in enumerate(j.rows.tolist()):
            v = [x & 0xFFFFFFFF for x in row[:6]]
            slot, sec = divmod(r, 6)
            slots.add(slot)
            for q in range(6):
                g[1 + q] += v[q]
            g[8] = max(g[8], min(v[0], 0xFFFFFFFE) + 1)
            b = slot * j.access_time // case.bin_ms
            if b >= case.bins:
                g[7] += v[0]
                continue
            for q in range(6):
                series[q][j.group][sec][b] += v[q]
        g[0] += len(slots)
    return np.array(series, dtype=np.int64), np.array(sc, dtype=np.int64)


def test_case_names(cases):
    assert tuple(cases) == N.CASE_NAMES


@pytest.mark.parametrize("name", [n for n in N.CASE_NAMES if n != "empty_group_many_jobs"])
def test_reference_equals_the_plain_loop(cases, name):
    assert N.same(cases[name].reference(), plain_loop(cases[name])) is None


def test_generator_is_deterministic():
    for x, y in zip(N.cases(), N.cases()):
        assert all(np.array_equal(p.rows, q.rows) for p, q in zip(x.jobs, y.jobs))


def test_cases_hold_what_they_are_for(cases):
    T = N.TILE
    assert {len(j.rows) for j in cases["tile_edges"].jobs} == {T - 1, T, T + 1, 1, 5, 6, 7}
    for name in ("huge_one_slot_per_bin", "huge_four_bins"):
        series, sc = cases[name].reference()
        assert int(series.max()) >= (2**32 if name == "huge_four_bins" else N.HUGE - 2) and int(sc[:, 1:7].min(axis=1).max()) > 2**32
    assert int(cases["huge_four_bins"].reference()[1][1, 7]) == 0 and int(cases["huge_four_bins"].reference()[0][:, 1, :, 3].min()) > 0  # four bins, all used, no overflow
    for name, exceeded in (("bin_below_slot_window_exceeded", True), ("bin_below_slot_and_overflow", True), ("bin_7_slot_5_and_10", True), ("bin_25", False),
                           ("tile_edges", False)):  # (7 ms bins lie below the 10 ms slots of one job of that case)
        c = cases[name]
        spans = [((min(len(j.rows), f + T) - 1) // 6 * j.access_time) // c.bin_ms - (f // 6 * j.access_time) // c.bin_ms + 1 for j in c.jobs for f in range(0, len(j.rows), T)]
        assert (max(spans) > N.WINDOW) == exceeded, (name, max(spans))
    assert cases["bin_below_slot_and_overflow"].reference()[1][:, 7].tolist()[0] > 0 == cases["bin_below_slot_and_overflow"].reference()[1][1, 7] and int(cases["bin_below_slot_window_exceeded"].reference()[1][:, 7].max()) == 0
    assert {j.access_time for j in cases["bin_7_slot_5_and_10"].jobs} == {5, 10} and 5 % 7 and 10 % 7
    series, sc = cases["everything_behind_the_last_bin"].reference()
    assert not series.any() and (sc[:, 7] == sc[:, 1]).all() and (sc[:, 1] > 0).all()
    series, sc = cases["all_zero"].reference()
    assert not series.any() and not sc[:, 1:8].any() and (sc[:, 8] == 1).all() and (sc[:, 0] > 0).all()
    series, sc = cases["empty_group_many_jobs"].reference()
    assert not sc[1].any() and not series[:, 1].any() and (sc[[0, 2], 1] > 0).all() and len(cases["empty_group_many_jobs"].jobs) == 300
    assert all((j.rows[:, 6:] == N.PATTERN).all() for c in cases.values() for j in c.jobs)  # two words that are not the kernel's to read


def test_harness_compiles_carries_the_constants_and_accepts_every_case(pkg, cases, tmp_path):
    """hipcc --offload-arch=gfx950 on the harness, which pulls in prach_noma_trace.hip as it is; --check reads and places a case without a HIP call."""
    exe = N.build_harness(tmp_path)
    assert N.harness_constants(exe) == N.CONSTANTS and pkg.noma_trace_tile_rows() == N.TILE == 6 * N.WINDOW
    for name, case in cases.items():
        path = str(tmp_path / f"{name}.bin")
        N.write_case(case, path)
        H.run(exe, ["--check", path], timeout=60)
    bad = str(tmp_path / "bad.bin")
    c = cases["all_zero"]
    N.write_case(N.Case("bad", 0, 5, 1, c.jobs[:1]), bad)
    with pytest.raises(H.Abnormal):
        H.run(exe, ["--check", bad], timeout=60)
