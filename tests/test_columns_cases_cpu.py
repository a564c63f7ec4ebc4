"""The synthetic cases of prach::columns_kernel without a GPU: the generator is deterministic and contains what it exists for, the numpy restatement equals
the host definition wherever a case's schedules are the product's own, and tests/tools/gpu_columns_harness.hip compiles for gfx950 and carries the
constants the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import columns_cases as CC  # noqa: E402
import reduce_cases as R  # noqa: E402
import xtab_ref as X  # noqa: E402


@pytest.fixture(scope="module")
def cases(pkg):
    return CC.cases(pkg)


def test_generator_is_deterministic_and_contains_what_it_exists_for(pkg, cases, tmp_path):
    again = CC.cases(pkg)
    assert tuple(c.name for c in cases) == CC.CASE_NAMES
    for a, b in zip(cases, again):
        assert a.fields == b.fields and all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and (x.E, x.lead) == (y.E, y.lead) for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    ref = {n: by[n].reference() for n in CC.CASE_NAMES}
    # sizes and offsets: 1, around a wavefront and a workgroup's stride, around the tile; every residue of the offsets mod 4 rows; 1 and 16 columns
    for name in ("sizes_all_menu", "sizes_all_raw", "one_column_arrival", "one_column_raw_timer", "sixteen_columns_mixed"):
        off, sc, data = ref[name]
        assert [j.nue for j in by[name].jobs] == list(CC.SIZES) and {1, 63, 64, 65, 8191, 8192, 8193} <= set(CC.SIZES)
        assert {int(o) % 4 for o in off} == {0, 1, 2, 3} and (sc[:, :3].sum(axis=1) == CC.SIZES).all() and (sc[:, 3] == 0).all()
        assert int(off[list(CC.SIZES).index(8192) + 1]) % 2 == 1  # an odd offset behind a tile edge
    assert len(by["one_column_arrival"].fields) == 1 and len(by["one_column_raw_timer"].fields) == 1 and len(by["sixteen_columns_mixed"].fields) == 16
    assert by["sizes_all_menu"].fields == CC.MENU and by["sizes_all_raw"].fields == CC.RAW and len(set(by["repeated_fields"].fields)) < len(by["repeated_fields"].fields)
    # the guards are there, in front of and behind every segment of every column
    c = by["sizes_all_menu"]
    off, sc, data = ref[c.name]
    for t, j in enumerate(c.jobs):
        assert (data[:, off[t] - j.lead:off[t]] == CC.FILL).all() and (data[:, off[t]:off[t] + j.nue] != CC.FILL).all()
    assert (data[:, -c.tail:] == CC.FILL).all()
    # undefined values of every kind: idle UEs, an E below an arrival, a completion before the arrival; INT_MIN and INT_MAX raw words
    j = c.jobs[-1]
    v = {f: X.values(f, j.logs, j.sched, j.access_time, j.E) for f in CC.MENU}
    arrived = j.logs[:, X.T.ACTIVE] != -1
    assert (v[X.AGE][arrived] < 0).any() and (v[X.AGE][arrived] >= 0).any() and (v[X.SOJOURN][v[X.STATE] == 1] < 0).any() and (v[X.TIMER][arrived] < 0).any()
    seg = data[:, off[-1]:off[-1] + j.nue]
    assert ((seg[X.AGE] == -1) & arrived).any() and ((seg[X.SOJOURN] == -1) & (v[X.STATE] == 1)).any() and set(np.unique(seg[X.STATE]).tolist()) == set(range(7))
    rawseg = ref["sizes_all_raw"][2]
    assert (rawseg == CC.INT_MIN).any() and (rawseg == CC.INT_MAX).any()
    big = by["sizes_all_menu"].jobs[-1].logs[:, X.T.TXTIME] == CC.INT_MAX  # a completion past int32: the low 32 bits, as the definition says
    assert big.any()
    # both sides of every threshold
    t = by["thresholds"].jobs[0]
    assert {tuple(r) for r in t.logs[:, [X.T.ACTIVE, X.T.FLAG, X.NOWBACKOFF, X.CONNREQ]].tolist()} >= {(act, m4, nb, cr) for act in (-1, 0, 1, 2) for m4 in (0, 1) for nb in (0, 1) for cr in (47, 48)}
    off, sc, data = ref["thresholds"]
    assert set(np.unique(data[X.STATE, off[0]:off[0] + t.nue]).tolist()) == set(range(7))
    # the slot range of a tile around TILE_SCHED_CAP
    assert [int(np.searchsorted(j.sched, j.nue - 1, side="right")) - int(np.searchsorted(j.sched, 0, side="right")) for j in by["schedules_around_the_staging_limit"].jobs] == \
        [CC.TILE_SCHED_CAP - 1, CC.TILE_SCHED_CAP, CC.TILE_SCHED_CAP + 1]
    sizes = [j.nue for j in by["very_different_sizes"].jobs]
    assert min(sizes) == 1 and max(sizes) >= 4 * CC.TILE
    assert not any(f in (X.ARRIVAL, X.SOJOURN, X.AGE, X.STATE, X.PTC) or CC.COL_RAW + 4 <= f < CC.COL_RAW + 12 for f in by["no_arrival_no_optional_quarters"].fields)
    f = by["raw_words_of_every_quarter"].fields  # the optional quarters are loaded for the raw words alone, next to a field that needs a(i)
    assert {(x - CC.COL_RAW) >> 2 for x in f if x >= CC.COL_RAW} == {0, 1, 2, 3} and {x for x in f if x < CC.COL_RAW} == {X.TIMER, X.AGE}
    p = str(tmp_path / "case.bin")
    CC.write_case(by["thresholds"], p)
    assert os.path.getsize(p) == 4 * (32 + 8 * 3 + sum(16 * j.nue + len(j.sched) for j in by["thresholds"].jobs))


def test_reference_equals_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert CC.same(host, ref) is None, (c.name, CC.same(host, ref))
        seen += 1
    assert seen == 1


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = CC.build_harness(tmp_path)
    assert R.harness_constants(exe) == CC.CONSTANTS
    assert CC.TILE == pkg.columns_tile_ues() and CC.COL_MAX == pkg.COL_MAX and CC.COL_RAW == pkg.COL_RAW and CC.NAMES == pkg.XTAB_FIELD_NAMES
