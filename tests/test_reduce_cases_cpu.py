"""tests/tools/reduce_cases.py without a GPU: for every generated case the host definition accepts, the numpy reference equals prach_dist_accumulate_logs /
prach_timeline_accumulate_logs on logs synthesised from the same arrays — which checks the generator and the references that
tests/test_gpu_reduce_synthetic.py holds the two kernels against; the generated cases contain what they are there for; and
tests/tools/gpu_reduce_harness.hip compiles for gfx950 and carries the constants the generator places its sizes around."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import reduce_cases as R  # noqa: E402
import timeline_ref as T  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return {c.name: c for c in R.dist_cases() + R.timeline_cases(pkg)}


def test_case_names(cases):
    assert tuple(cases) == R.DIST_CASE_NAMES + R.TIMELINE_CASE_NAMES


@pytest.mark.parametrize("name", R.DIST_CASE_NAMES + R.TIMELINE_CASE_NAMES)
def test_reference_equals_the_host_definition(pkg, cases, name):
    case = cases[name]
    ref = case.reference()
    if case.kind == "dist":
        assert int(ref.trials.sum()) == len(case.jobs) and int(ref.ues.sum()) == sum(j.nue for j in case.jobs)
    else:
        assert int(ref.series["arrivals"].sum()) + int(ref.scalars["arrival_overflow"].sum()) == int(ref.scalars["arrived"].sum())
        assert int(ref.series["done"].sum()) + int(ref.scalars["done_overflow"].sum()) == int(ref.scalars["success"].sum())
        tl = T.numpy_timeline(pkg, [j.logs for j in case.jobs], [j.sched for j in case.jobs], [j.access_time for j in case.jobs], case.bins, case.width,
                              [j.group for j in case.jobs], case.ngroups)
        assert case.same(ref, tl) is None  # (the restatement the engine tests use is this one)
    if not case.host:
        assert case.kind == "timeline" and any(j.cfg_kw is None for j in case.jobs)
        return
    if case.kind == "timeline":  # the schedule each job carries is the product's own for its config
        for j in case.jobs:
            assert pkg.arrival_schedule(pkg.make_cfg(j.nue, rng_mode=pkg.RNG_PHILOX, **j.cfg_kw))[0] == j.sched.tolist()
    assert case.same(ref, case.host_definition(pkg)) is None


def test_generator_is_deterministic():
    a, b = R.dist_cases(), R.dist_cases()
    for x, y in zip(a, b):
        assert all(np.array_equal(p.timers, q.timers) and np.array_equal(p.data, q.data) for p, q in zip(x.jobs, y.jobs))


def test_dist_cases_hold_what_they_are_for(cases):
    main = cases["dist_sizes_shares_patterns"]
    assert {j.nue for j in main.jobs} == set(range(1, 10)) | {R.TILE - 1, R.TILE, R.TILE + 1, 3 * R.TILE + 1, 3 * R.TILE + 2, 3 * R.TILE + 3}
    assert {j.nue % 4 for j in main.jobs if j.nue > 3 * R.TILE} == {1, 2, 3} and {j.nue % 4 for j in main.jobs if j.nue < 10} == {0, 1, 2, 3}
    ref = main.reference()
    assert ref.ptc_hist[:, 255].sum() > 1000 and ref.ptc_hist[:, 254].sum() > 100  # the clamp and the bin below it
    assert int(ref.delay_sum.max()) > 2**44 - 2**34 and int(ref.delay_max.max()) == R.INT_MAX and int(ref.delay_overflow.sum()) > 0
    high = [j for j in main.jobs if j.form == 1 and (j.data[:, 5] >> 16).any()]
    assert high and any((j.data[:, 5] < 0).any() for j in high)  # a high half in word 5, also with its top bit set
    for j in main.jobs:
        ok = j.timers != R.INT_MIN
        if j.form == 1:
            assert (j.data[~ok] == R.PATTERN).all()
        else:
            assert (j.data[~ok] != 0).all()
    # 64 distinct values in one wavefront: lanes 0..63 of a wavefront hold UEs 4 lane + c of every 1024-UE stretch
    j = next(j for j in main.jobs if j.nue == R.TILE and j.form == 0 and (j.timers != R.INT_MIN).all() and len(np.unique(j.data[:256:4])) == 64)
    assert all(len(np.unique(j.data[c:256:4])) == 64 for c in range(4))
    assert {(c.bins, c.width) for c in cases.values() if c.kind == "dist"} == {(1023, 7), (1, 1), (2, 3), (16384, 1), (16, 1 << 20)}
    many = cases["dist_2000_jobs_7_groups"]
    assert len(many.jobs) == 2000 and many.ngroups == 7 and {j.group for j in many.jobs} == {0, 1, 3, 4, 6}
    assert sum(j.nue > R.TILE for j in many.jobs) >= 4 and sum(j.nue <= 300 for j in many.jobs) > 1900


def test_timeline_cases_hold_what_they_are_for(cases):
    def slot_range(j, tile):
        first, last = tile * R.TILE, min(j.nue, (tile + 1) * R.TILE) - 1
        return int(np.searchsorted(j.sched, last, side="right") - np.searchsorted(j.sched, first, side="right"))
    rng = cases["timeline_schedule_ranges"]
    spans = [slot_range(j, t) for j in rng.jobs for t in range(-(-j.nue // R.TILE))]
    assert {R.SCHED_CAP - 1, R.SCHED_CAP, R.SCHED_CAP + 1} <= set(spans) and 0 in spans
    assert any(j.sched[-1] < R.TILE and j.nue > R.TILE and (j.logs[R.TILE:, R.ACTIVE] != -1).any() for j in rng.jobs)  # a schedule that ends below a tile
    assert any((j.logs[R.TILE:2 * R.TILE, R.ACTIVE] == -1).all() for j in rng.jobs if j.nue >= 2 * R.TILE)  # a tile in which no UE has arrived
    one = cases["timeline_one_slot_sojourn_sums"].reference()
    assert int(one.series["sojourn_sum"].max()) == R.TILE << 20 > 2**32 and int(one.series["success"].max()) == R.TILE
    assert sorted(int(v) // R.TILE for v in one.scalars["sojourn_sum"]) == [0, R.MAX_SOJOURN, R.MAX_SOJOURN + 1, 1 << 20, 1 << 20]
    above = cases["timeline_timer_above_sojourn"]
    assert above.host and int(above.reference().series["timer_sum"].max()) >= R.TILE << 20
    assert any(((j.logs[:, R.TIMER] == 1 << 20) & (j.logs[:, R.TXTIME] + 6 - R.arrival_times(j.nue, j.sched, j.access_time) == 100)).all() for j in above.jobs)
    for name in R.TIMELINE_CASE_NAMES:
        if not name.startswith("timeline_window_edges"):
            continue
        c = cases[name]
        j = c.jobs[0]
        at = R.arrival_times(j.nue, j.sched, 1)
        ok = (j.logs[:, R.FLAG] == 1) & (j.logs[:, R.ACTIVE] != -1)
        ab, db = at[ok] // c.width, (j.logs[ok, R.TXTIME].astype(np.int64) + 6) // c.width
        b0 = int(at[0]) // c.width
        pairs = set(zip(ab.tolist(), db.tolist()))
        want = {b for b in (b0 + R.WINDOW - 1, b0 + R.WINDOW, c.bins - 1, c.bins) if b >= b0}
        assert want <= set(ab.tolist()) and want <= set(db.tolist())
        assert any(a - b0 < R.WINDOW and d - b0 >= R.WINDOW for a, d in pairs)  # done outside the window, arrival inside
    assert {(c.bins, c.width) for c in cases.values() if c.kind == "timeline"} >= {(1, 1), (2002, 1), (2002, 3), (65536, 1), (65536, 3)}
    many = cases["timeline_1500_jobs_5_groups"]
    assert len(many.jobs) == 1500 and many.ngroups == 5 and {j.group for j in many.jobs} == set(range(5))
    real = cases["timeline_real_schedules_bins2002_width3"]
    assert {(j.cfg_kw["uniform"], j.cfg_kw["accessTime"]) for j in real.jobs} == {(0, 5), (0, 7), (1, 1)}


def test_harness_compiles_and_carries_the_generators_constants(pkg, tmp_path):
    """hipcc --offload-arch=gfx950 on the harness, which pulls in prach_dist.hip and prach_timeline.hip as they are; nothing is launched."""
    exe = R.build_harness(tmp_path)
    assert R.harness_constants(exe) == R.CONSTANTS
    assert (R.TILE, R.PTC_BINS, R.WINDOW, R.MAX_SOJOURN, R.SCHED_CAP) == tuple(R.CONSTANTS[k] for k in ("DIST_TILE", "DIST_PTC_BINS", "TL_WINDOW", "TL_MAX_SOJOURN",
                                                                                                          "TL_SCHED_CAP"))
    assert pkg.dist_tile_ues() == R.CONSTANTS["DIST_TILE"] and pkg.timeline_tile_ues() == R.CONSTANTS["TL_TILE"] == R.TILE
    assert pkg.timeline_window_bins() == R.WINDOW
