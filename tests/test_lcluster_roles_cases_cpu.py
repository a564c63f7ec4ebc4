"""The exchange roles of prach::lcluster_kernel, their cases without a GPU (tests/tools/roles_cases.py): the shapes make live what they are there for,
and from the oracle's census every trial (both variants, both RNG modes) holds at least three dozen subframes with calls, with singleton calls and with
UEs that leave their bucket — a bucket granule, an event granule and a grant in many subframes, so that a green run of tests/test_gpu_lcluster_roles.py
means the repacked roles carried them.  Conditions on the CASES, not measurements of the library."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import roles_cases as RC  # noqa: E402

FEW_DOZEN = 36


def test_shapes_make_the_roles_live():
    lv = {name: RC.live(name) for name, _, _, _ in RC.CASES}
    assert lv["g24_p54"] == dict(bucket_roles=2, tail=False, ev1=False)
    assert lv["g40_p54"] == dict(bucket_roles=3, tail=False, ev1=True)
    assert lv["g64_p54"] == dict(bucket_roles=3, tail=True, ev1=True)
    assert lv["g64_p8"] == dict(bucket_roles=1, tail=False, ev1=True)
    assert lv["g64_p64"] == dict(bucket_roles=3, tail=True, ev1=True)
    assert lv["g32_p54"] == dict(bucket_roles=2, tail=False, ev1=False)
    for name, G, n, kw in RC.CASES:
        assert 64 * G <= n <= 3 * 64 * G + 64, (name, "every workgroup owns a group, and the trial stays small")
        assert 3 <= kw["nGrantUL"] <= 6 and kw["nPreamble"] <= 64 and G <= 64
        assert max(RC.CUTS) < 10000 and {(c - 1) % 5 for c in RC.CUTS} == set(range(5))


@pytest.mark.parametrize("rng", [0, 1])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", [c[0] for c in RC.CASES])
def test_trial_holds_calls_singletons_and_leavers(ob, name, variant, rng):
    c = RC.census(name, variant, rng)
    got = RC.counts(c)
    print(name, variant, rng, "subframes with calls / singleton calls / leavers:", got, "of", c["steps"], "; successes", c["nSuccessUE"])
    assert min(got.values()) >= FEW_DOZEN, got
    assert c["steps"] > max(RC.CUTS), "every cut stops a running trial"
