"""The frame of the off-trial kernel harnesses (tests/tools/harness_frame.h, tests/tools/harness.py) without a GPU: each of the eight programs that read a
job case file accepts every case its family generates (`PROGRAM --check CASE`: everything up to and including placement, no HIP call) and refuses a
malformed file with exit status 3, under --check and on the way to a launch alike.  Every exit here happens before the first HIP call."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import columns_cases as CC  # noqa: E402
import harness as H  # noqa: E402
import noma_census_cases as NC  # noqa: E402
import noma_census_ref as N  # noqa: E402
import noma_select_cases as NS  # noqa: E402
import noma_select_ref as S  # noqa: E402
import pick_cases as PC  # noqa: E402
import pick_ref as P  # noqa: E402
import reduce_cases as R  # noqa: E402
import sojourn_cases as SJ  # noqa: E402
import summary_cases as SM  # noqa: E402
import xtab_cases as XC  # noqa: E402

NUE, SCHED = 3, [1, 3]  # the smallest case of every program: one job of three UEs, two access slots
LOGS = np.arange(NUE * 16, dtype=np.int32).reshape(NUE, 16)
AXES = ((0, 1, 1), (0, 1, 1), 1)  # field ONE on both axes, one bin each, the first class: in range for the trial menu and the NOMA menu alike

# family -> (module, every generated case, the arguments behind `--check CASE`)
FAMILIES = {
    "reduce_dist": (R, lambda pkg: R.dist_cases(), [[]]), "reduce_timeline": (R, R.timeline_cases, [[]]), "sojourn": (SJ, SJ.cases, [[]]), "summary": (SM, SM.cases, [[]]),
    "xtab": (XC, XC.cases, [[]]), "pick": (PC, PC.cases, [[]]), "columns": (CC, CC.cases, [[]]), "noma_census": (NC, NC.cases, [[], ["columns"]]),
    "noma_select": (NS, NS.cases, [[]]),
}
# program (and kind of file) -> (module, its smallest case, header words, the arguments behind `--check CASE`, the arguments behind `CASE RESULT`)
SMALLEST = {
    "reduce_dist": (R, lambda: R.Case("dist", "mini", 8, 1, 1, [R.DistJob([5, R.INT_MIN, 7], 0, [1, 2, 3], 0)], True), 16, [[]], [[0]]),
    "reduce_timeline": (R, lambda: R.Case("timeline", "mini", 8, 1, 1, [R.TimelineJob(LOGS, SCHED, 5, 0)], False), 16, [[]], [[0]]),
    "sojourn": (SJ, lambda: SJ.Case("mini", (4, 5, 8, 100), 1, [R.TimelineJob(LOGS, SCHED, 5, 0)], False), 16, [[]], [[0]]),
    "summary": (SM, lambda: SM.Case("mini", (500,), [R.TimelineJob(LOGS, SCHED, 5, 0)]), 16, [[]], [[512]]),
    "xtab": (XC, lambda: XC.Case("mini", AXES, 1, [XC.Job(LOGS, SCHED, 5, 0, 9)], False), 16, [[]], [[0]]),
    "pick": (PC, lambda: PC.Case("mini", (), P.BY_INDEX, 0, 4, 1, [PC.Job(LOGS, SCHED, 5, 9)]), 32, [[]], [[512]]),
    "columns": (CC, lambda: CC.Case("mini", [0], [CC.Job(LOGS, SCHED, 5, 9)]), 32, [[]], [[]]),
    "noma_census": (NC, lambda: NC.Case("mini", AXES, 1, [NC.Job(LOGS, SCHED, 5, 0, 9)], False), 32, [[], ["columns"]], [["census", 0], ["columns"]]),
    "noma_select_summary": (NS, lambda: NS.Case("summary_mini", ((N.ONE,), 1, (500,)), [NC.Job(LOGS, SCHED, 5, 0, 9)], False), 32, [[]], [[512]]),
    "noma_select_pick": (NS, lambda: NS.Case("pick_mini", ((), S.BY_INDEX, N.ONE, 4, 1), [NC.Job(LOGS, SCHED, 5, 0, 9)], False), 32, [[]], [[512]]),
}
LOG_ONLY = ("schedule_decreases", "nslots_0")  # what a dist job does not have
MALFORMATIONS = ("truncated", "trailing_word", "wrong_magic", "njobs_0", "group_out_of_range", "length_not_a_multiple_of_4") + LOG_ONLY


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """The eight programs, compiled side by side; {module: executable}."""
    d = tmp_path_factory.mktemp("harness_frame")
    mods = (R, SJ, SM, XC, PC, CC, NC, NS)
    with ThreadPoolExecutor(len(mods)) as pool:
        return dict(zip(mods, pool.map(lambda m: m.build_harness(d), mods)))


def malformed(words, head, what):
    """The bytes of the smallest case's file with one thing wrong."""
    a = words.copy()
    if what == "truncated":
        a = a[:-2]
    elif what == "trailing_word":
        a = np.append(a, np.int32(0))
    elif what == "wrong_magic":
        a[0] ^= 1
    elif what == "njobs_0":
        a[2] = 0
    elif what == "group_out_of_range":
        a[head + 1] = 7
    elif what == "schedule_decreases":
        a[-2:] = SCHED[::-1]
    elif what == "nslots_0":
        a[head + 4] = 0
    return a.tobytes() + (b"\0" if what == "length_not_a_multiple_of_4" else b"")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_generated_case_passes_check(pkg, exes, tmp_path, family):
    mod, generate, checks = FAMILIES[family]
    cases = generate(pkg)
    assert cases
    path = str(tmp_path / "case.bin")
    for case in cases:
        mod.write_case(case, path)
        for extra in checks:
            p = H.run(exes[mod], ["--check", path, *extra], ok=(0, 3))
            assert p.returncode == 0, (case.name, extra, p.stderr)
    os.remove(path)


@pytest.mark.parametrize("program,what", [(p, w) for p in SMALLEST for w in MALFORMATIONS if not (p == "reduce_dist" and w in LOG_ONLY)])
def test_malformed_file_is_refused_with_exit_3(exes, tmp_path, program, what):
    mod, smallest, head, checks, launches = SMALLEST[program]
    good, bad, res = str(tmp_path / "good.bin"), str(tmp_path / "bad.bin"), str(tmp_path / "result.bin")
    mod.write_case(smallest(), good)
    words = np.fromfile(good, dtype="<i4")
    assert words.size == head + 8 + (2 * NUE if program == "reduce_dist" else 16 * NUE + len(SCHED))
    with open(bad, "wb") as f:
        f.write(malformed(words, head, what))
    for extra in checks:
        assert H.run(exes[mod], ["--check", good, *extra]).returncode == 0  # (what is refused below is refused for the one thing wrong with it)
        p = H.run(exes[mod], ["--check", bad, *extra], ok=(0, 2, 3))
        assert p.returncode == 3 and p.stderr.startswith(os.path.basename(exes[mod]) + ": "), (p.returncode, p.stderr)
    for own in launches:  # on the way to a launch the same file is refused before the first HIP call
        p = H.run(exes[mod], [bad, res, *own], ok=(0, 2, 3))
        assert p.returncode == 3 and not os.path.exists(res), (p.returncode, p.stderr)
