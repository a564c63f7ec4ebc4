"""The synthetic cases of prach::pick_kernel without a GPU: the generator is deterministic and reaches the states it is there for, the numpy restatement of
the kernel's raw output equals the host definition wherever a case's schedules are the product's own, and tests/tools/gpu_pick_harness.hip compiles for
gfx950 and carries the constants the generator assumes."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import pick_cases as PC  # noqa: E402
import reduce_cases as R  # noqa: E402

SELECTED, MATCHED, STORED, UNDEFINED, RERR, THRESHOLD, TIES = range(7)  # the scalars
KEY = 17  # word of a row


@pytest.fixture(scope="module")
def cases(pkg):
    return PC.cases(pkg)


def test_generator_is_deterministic_and_reaches_its_states(pkg, cases, tmp_path):
    again = PC.cases(pkg)
    assert tuple(c.name for c in cases) == PC.CASE_NAMES
    for a, b in zip(cases, again):
        assert all(np.array_equal(x.logs, y.logs) and np.array_equal(x.sched, y.sched) and x.E == y.E for x, y in zip(a.jobs, b.jobs))
    by = {c.name: c for c in cases}
    ref = {n: by[n].reference() for n in PC.CASE_NAMES}
    for name in ("sizes_by_index", "sizes_largest_timer"):
        sc, rows = ref[name]
        assert [j.nue for j in by[name].jobs[:len(PC.SIZES)]] == list(PC.SIZES) and {511, 512, 513, 1023, 1024, 1025, 2049} <= set(PC.SIZES)
        assert (sc[:, STORED] == np.minimum(sc[:, MATCHED], 7)).all() and (sc[:, STORED] == 7).sum() >= 8 and not sc[:, RERR].any()
    sc, rows = ref["sizes_by_index"]
    idle_only, nobody_served = len(PC.SIZES), len(PC.SIZES) + 1
    assert sc[idle_only, SELECTED] == 700 == sc[idle_only, MATCHED] and (rows[idle_only, :, 16] == -1).all() and (sc[:, THRESHOLD] == -1).all() and not sc[:, TIES].any()
    sc, rows = ref["sizes_largest_timer"]
    assert sc[idle_only, MATCHED] == 0 and sc[idle_only, UNDEFINED] == 700 and sc[idle_only, THRESHOLD] == -1 and (rows[idle_only] == PC.FILL).all() and sc[nobody_served, MATCHED] > 7
    assert (sc[:len(PC.SIZES), UNDEFINED] > 0).sum() >= 8  # an age behind E, an idle UE
    for name, k in (("k_1", 1), ("k_matched_minus_1", PC.MATCHED - 1), ("k_matched", PC.MATCHED), ("k_matched_plus_1", PC.MATCHED + 1)):
        sc, rows = ref[name]
        assert (sc[:, MATCHED] == PC.MATCHED).all() and (sc[:, STORED] == min(k, PC.MATCHED)).all() and by[name].k == k
        assert (sc[:, TIES] > 0).any() == (k < PC.MATCHED) and ((rows[:, -1] == PC.FILL).all(axis=1) == (k > PC.MATCHED)).all()
    sc, rows = ref["k_max"]
    assert by["k_max"].k == PC.MAX_K and sc[:, MATCHED].tolist()[1:3] == [4097, 4096] and (sc[:, STORED] == PC.MAX_K).sum() == 4 and sc[3, MATCHED] < PC.MAX_K and sc[0, TIES] > 0
    sc, rows = ref["all_keys_equal_and_ties_across_blocks"]
    assert sc[0].tolist() == [2100, 2100, 1100, 0, 0, 777, 1000, 0] and rows[0, :, 0].tolist() == list(range(1100))  # the first k by index
    assert sc[2, THRESHOLD] == 8 and sc[2, TIES] > 0 and (rows[2, :, KEY] == 9).sum() == 32 and sc[3].tolist()[2:] == [1100, 0, 0, 3, 1000, 0] and rows[3, [29, 30, -1], 0].tolist() == [29, 1030, 2099]
    assert sc[4].tolist()[1:7] == [1100, 1100, 0, 0, 1, 0] and sc[5].tolist()[1:7] == [1099, 1099, 0, 0, 1, 0] and (rows[5, -1] == PC.FILL).all()
    for name, other in (("thresholds_largest", 0), ("thresholds_smallest", 65535)):
        sc, rows = ref[name]
        assert {0, 63, 64, 64511, 64512, 65535} <= set(sc[:, THRESHOLD].tolist()) and (sc[:, STORED] == 50).all() and not sc[:, RERR].any()
        assert {0, 3} <= set(sc[:, TIES].tolist()) and sc[:, TIES].max() >= 1250
    sc, rows = ref["one_key_65536"]
    assert sc[:, RERR].tolist() == [1, 70, 0] and sc[:, MATCHED].tolist() == [1000, 70, 300] and sc[:, STORED].tolist() == [16, 0, 16] and rows[0, :, KEY].max() <= 3000
    assert sc[1, THRESHOLD] == -1 and (rows[1] == PC.FILL).all()
    for f, n in enumerate(PC.NAMES):
        c = by[f"key_{n}"]
        sc, rows = ref[c.name]
        assert c.key == f and len(c.where) == 3 and (sc[:, MATCHED] > 0).sum() >= 3 and not sc[:, RERR].any(), c.name
    assert {g for n in PC.NAMES for g, _, _ in by[f"key_{n}"].where} == set(range(9))  # every field is a clause somewhere
    c = by["schedule_around_the_staging_limit"]
    assert [len(j.sched) for j in c.jobs] == [PC.SCHED_CAP, PC.SCHED_CAP + 1] and (ref[c.name][0][:, STORED] == 40).all()
    sc, rows = ref["real_schedules"]
    assert sorted({j.nue for j in by["real_schedules"].jobs}) == [1, 65, 1025, 8193] and any(len(j.sched) > PC.SCHED_CAP for j in by["real_schedules"].jobs) and (sc[:, STORED] == 64).sum() >= 4
    p = str(tmp_path / "case.bin")
    PC.write_case(by["k_1"], p)
    assert os.path.getsize(p) == 4 * (32 + 8 * len(by["k_1"].jobs) + sum(16 * j.nue + len(j.sched) for j in by["k_1"].jobs))


def test_reference_equals_the_host_definition(pkg, cases):
    seen = 0
    for c in cases:
        if not c.host:
            continue
        ref, host = c.reference(), c.host_definition(pkg)
        assert PC.same(host, ref) is None, (c.name, PC.same(host, ref))
        seen += 1
    assert seen == 1


def test_harness_compiles_and_carries_the_constants(pkg, tmp_path):
    exe = PC.build_harness(tmp_path)
    assert R.harness_constants(exe) == PC.CONSTANTS
    assert PC.CONSTANTS["PK_MAX_KEY"] == pkg.summary_max_value() == PC.MAX_KEY and PC.MAX_K == pkg.PICK_MAX_K and 8 * PC.ROW_WORDS == pkg.pick_row_dtype().itemsize
