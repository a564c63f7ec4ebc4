"""The synthetic cases of prach::noma_timeline_kernel without a GPU: the generator is deterministic and reaches the states it is there for, the numpy
restatement equals the host definition wherever a case's schedules are the product's own, and tests/tools/gpu_noma_timeline_harness.hip compiles for gfx950,
accepts every case under --check, refuses malformed files with exit code 3 and carries the constants the generator assumes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import noma_census_ref as N  # noqa: E402
import noma_timeline_cases as TC  # noqa: E402
import noma_timeline_ref as T  # noqa: E402
import reduce_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return TC.cases(pkg)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return TC.build_harness(tmp_path_factory.mktemp("noma_timeline_harness"))


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases):
    again = TC.cases(pkg)
    assert tuple(c.name for c in cases) == TC.CASE_NAMES
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and x.E == y.E and x.group == y.group for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    refs = {c.name: c.reference() for c in cases}
    assert all(T.identity(r) for r in refs.values())
    W, TILE, MAXS = TC.WINDOW, TC.TILE, TC.MAX_SOJOURN

    c = by["real_sizes_wild_records"]
    assert sorted(j.nue for j in c.jobs) == [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    logs = np.concatenate([j.logs for j in c.jobs])
    cls = N.classes(logs)
    arrived, sv = cls != N.IDLE, cls == N.SERVED
    assert set(np.unique(cls)) == {N.SERVED, N.PENDING, N.IDLE, N.DROPPED}
    assert set(np.unique(np.concatenate([N.states(j.logs, j.E) for j in c.jobs]))) == set(range(9))  # every STATE, 8 too
    assert {6, TC.INT_MIN, 7, -2} <= set(logs[arrived, N.W_SECTOR].tolist()) and (logs[~arrived, N.W_RA] == 1).any()  # sector -1 is idle by definition, with a set RA
    assert (logs[sv, N.W_TIMER] < 0).any() and (logs[sv, N.W_TXTIME] < 0).any()
    r = refs[c.name]["scalars"]
    assert (r["undefined"] > 0).all() and (r["restarted"] > 0).all() and r["arrival_overflow"].sum() == 0 and (refs[c.name]["series"].sum(axis=(1, 2, 3)) > 0).all()
    r = refs["real_sizes_one_bin"]
    assert r["series"].shape == (6, 2, 6, 1) and int(r["scalars"]["arrival_overflow"].sum()) == 0 and int(r["scalars"]["done_overflow"].sum()) > 0

    c = by["budget_sojourn_and_timer"]
    a = c.jobs[0].logs.astype(np.int64)
    sj, tm = a[:, N.W_TXTIME] + 6 - 20, a[:, N.W_TIMER]
    assert {(MAXS, 0), (MAXS + 1, 0), (MAXS, MAXS), (MAXS + 1, MAXS + 1), (0, MAXS), (0, MAXS + 1), (2 ** 31 - 21, 5), (5, 2 ** 31 - 1)} <= set(zip(sj.tolist(), tm.tolist()))
    r = refs[c.name]
    assert int(r["scalars"]["served"][0]) == TILE + 3 == int(r["series"][T.SERVED].sum()) and int(r["scalars"]["done_max"][0]) == 2 ** 31 - 1
    assert int(r["series"][T.SOJOURN_SUM].sum()) == int(sj.sum()) > 2 ** 31 and int(r["scalars"]["timer_sum"][0]) == int(tm.sum()) > 2 ** 31

    r = refs["whole_tile_one_cell"]
    n = 2 * TILE + 1
    assert int(r["series"][T.ARRIVALS, 0, 3, 0]) == n == int(r["series"][T.ARRIVALS].sum()) and int(r["series"][T.SOJOURN_SUM, 0, 3, 0]) == n * MAXS == int(r["series"][T.TIMER_SUM, 0, 3, 0])
    assert TILE * MAXS < 2 ** 32 and int(r["series"][T.DONE, 0, 3, MAXS // 5]) == n and int(r["scalars"]["restarted"][0]) == 0

    c = by["window_spans_and_completions"]
    for g, (j, span) in enumerate(zip(c.jobs, (W - 1, W, W + 1))):
        ab = R.arrival_times(j.nue, j.sched, 1) // c.bin_ms
        assert j.nue == TILE and int(ab[0]) == 11 + g and int(ab[-1]) - int(ab[0]) + 1 == span
        done = refs[c.name]["series"][T.DONE, g].sum(axis=0)
        assert done[int(ab[0]) + W - 1] > 20 and done[int(ab[0]) + W] > 20  # the last bin of the window and the first behind it
    assert (refs[c.name]["series"][T.ARRIVALS, 2].sum(axis=0)[13 + W] > 0)  # an arrival bin behind the window

    c = by["last_bin_edges"]
    j = c.jobs[0]
    at = R.arrival_times(j.nue, j.sched, 1)
    edge = c.bins * c.bin_ms
    ok = (N.classes(j.logs) != N.IDLE) & (j.logs[:, N.W_SECTOR] >= 0)
    assert (at[ok] == edge - 1).any() and (at[ok] == edge).any()
    cc = j.logs[:, N.W_TXTIME].astype(np.int64) + 6
    dsv = (N.classes(j.logs) == N.SERVED) & (cc >= at) & (j.logs[:, N.W_TIMER] >= 0)
    assert (cc[dsv] == edge - 1).any() and (cc[dsv] == edge).any()
    r = refs[c.name]
    assert int(r["scalars"]["arrival_overflow"][0]) > 0 and int(r["scalars"]["done_overflow"][0]) > 0 and r["series"][T.ARRIVALS, 0, :, -1].sum() > 0 and r["series"][T.DONE, 0, :, -1].sum() > 0

    c = by["tiles_nobody_activated"]
    j = c.jobs[0]
    assert (N.classes(j.logs[TILE:2 * TILE]) == N.IDLE).all() and j.sched[-1] == 2 * TILE and (N.classes(j.logs[2 * TILE:]) != N.IDLE).any()
    r = refs[c.name]["series"][T.ARRIVALS]
    assert c.jobs[1].sched[-1] == 0 and r[0, :, 2000].sum() > 0 and r[1, :, 20].sum() == r[1].sum() > 0  # (a UE no slot activates arrives behind every slot: 5 x nslots)

    j = by["long_schedule_range"].jobs[0]
    at = R.arrival_times(j.nue, j.sched, 1)
    assert int(at[TILE - 1] - at[0]) > TC.CONSTANTS["TILE_SCHED_CAP"]
    c = by["jobs_1500_groups_3"]
    assert len(c.jobs) == 1500 and c.ngroups == 3 and {j.group for j in c.jobs} == {0, 1, 2}


def test_references_equal_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert TC.same(host, ref) is None, (c.name, TC.same(host, ref))
        seen += 1
    assert seen == 2


def test_harness_checks_every_case_and_refuses_malformed_files(cases, harness, tmp_path):
    good = None
    for c in cases:
        p = str(tmp_path / f"{c.name}.bin")
        TC.write_case(c, p)
        H.run(harness, ["--check", p], timeout=60)
        good = good or p
    raw = np.fromfile(good, dtype="<i4")

    def refused(words, name, nbytes=None):
        p = str(tmp_path / f"bad_{name}.bin")
        b = np.ascontiguousarray(words, dtype="<i4").tobytes()
        with open(p, "wb") as f:
            f.write(b if nbytes is None else b[:nbytes])
        r = subprocess.run([harness, "--check", p], capture_output=True, text=True, timeout=60)
        assert r.returncode == 3 and "gpu_noma_timeline_harness" in r.stderr, (name, r.returncode, r.stderr)

    def patched(at, v):
        w = raw.copy()
        w[at] = v
        return w

    refused(raw[:-1], "truncated")
    refused(np.append(raw, 0), "trailing")
    refused(raw, "odd_length", nbytes=raw.nbytes - 2)
    refused(patched(0, 1), "magic")
    refused(patched(1, 1), "kind")
    refused(patched(2, 0), "njobs")
    for at, v, name in ((3, 0, "bins0"), (3, 65537, "bins"), (4, 0, "bin_ms"), (5, 0, "ngroups0"), (5, 65, "ngroups"), (6, -1, "window_neg"), (6, TC.CONSTANTS["NTL_WINDOW_MAX"] + 1, "window")):
        refused(patched(at, v), name)
    row = 16  # the first job row: nUE, group, form, accessTime, nslots, E
    for at, v, name in ((row, 0, "nue"), (row + 1, 4, "group"), (row + 1, -1, "group_neg"), (row + 3, 0, "access_time"), (row + 4, 0, "nslots"), (row + 5, -1, "E")):
        refused(patched(at, v), name)
    njobs = int(raw[2])
    sched0 = 16 + 8 * njobs + 16 * int(raw[row])  # the first job's schedule
    refused(patched(sched0, int(raw[row]) + 1), "schedule")
    r = subprocess.run([harness, good, str(tmp_path / "r"), "2"], capture_output=True, text=True, timeout=60)  # (a scheme out of range is refused before any HIP call)
    assert r.returncode == 3


def test_harness_carries_the_constants(pkg, harness):
    assert R.harness_constants(harness) == TC.CONSTANTS
    assert TC.CONSTANTS["TL_TILE"] == pkg.noma_timeline_tile_ues() and TC.CONSTANTS["NTL_WINDOW"] == pkg.noma_timeline_window_bins()
    assert TC.CONSTANTS["TL_TILE"] * TC.CONSTANTS["NTL_MAX_SOJOURN"] < 2 ** 32
