"""The device rand() stream generator and the device activeUE on inputs no trial feeds them: tests/tools/gpu_stream_act_harness.hip runs
launch_glibc_stream_jobs / launch_glibc_stream (csrc/prach_stream.hip) on the job tables and noma_active_ue (csrc/prach_noma_act.h) on the draw lists of
tests/tools/stream_act_cases.py, one child process per launch, six in all.  Stream: every output word equals libc's rand() (the host's sequential
generator past 200 000 values), every guard word behind an output and every gap byte of the arena is untouched, a job gives the same words alone and among
fourteen others, and windows 2^32 and 2^40 values into a seed's stream continue each other.  activeUE: preamble, sector and draw count equal the host's
prach_noma_activation_stream on every case, the gain of every unflagged case lies within ACT_GAIN_ULP_ASSERTED ulps of the host libm's, every case the host
libm puts within ACT_BAND / 2 of a float rounding boundary is flagged, and at most 1 in 10^5 of the near misses and of 200 000 random UEs is.
tests/test_stream_act_cases_cpu.py holds the cases and references without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import stream_act_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


def _child(exe, case, res):
    with latch.child(os.path.basename(case)):
        S.run_harness(exe, case, res, timeout=120)


def stream_launch(exe, pkg, consts, jobs, d, tag, mode=1):
    case, res = str(d / f"{tag}.case"), str(d / f"{tag}.result")
    wins = S.write_stream_case(case, jobs, S.seeds_fn(pkg), consts["STREAM_CHUNK"], mode=mode)
    _child(exe, case, res)
    return S.read_stream_result(res, jobs, wins, consts, mode=mode)  # (asserts the guard words, the gaps and the windows)


def act_launch(exe, A, d, tag):
    case, res = str(d / f"{tag}.case"), str(d / f"{tag}.result")
    S.write_act_case(case, A)
    _child(exe, case, res)
    return S.read_act_result(res, len(A))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return S.build_harness(tmp_path_factory.mktemp("stream_act_harness"))


@pytest.fixture(scope="module")
def consts(exe):
    return S.harness_constants(exe)


@pytest.fixture(scope="module")
def host(pkg):
    return S.Host(pkg)


# ---- the stream ----
@pytest.fixture(scope="module")
def mixed(exe, pkg, consts, tmp_path_factory):
    jobs = S.mixed_jobs(consts["STREAM_CHUNK"])
    return jobs, stream_launch(exe, pkg, consts, jobs, tmp_path_factory.mktemp("mixed"), "mixed")


def check_mixed(pkg, jobs, out):
    for j in jobs:
        S.assert_stream_equal(f"{j['name']} (seed {j['seed']}, first {j['first']}, n {j['n']})", out[j["name"]], S.reference_stream(pkg, j["seed"], j["first"], j["n"]))


def test_stream_jobs_of_every_length_in_one_launch(pkg, mixed):
    jobs, out = mixed
    check_mixed(pkg, jobs, out)


def test_stream_job_alone_equals_itself_in_the_mix(exe, pkg, consts, mixed, tmp_path):
    jobs, out = mixed
    for k, j in enumerate((S.longest_job(consts["STREAM_CHUNK"]),)):
        alone = stream_launch(exe, pkg, consts, [j], tmp_path, f"alone{k}")[j["name"]]
        S.assert_stream_equal(j["name"] + " alone", alone, S.reference_stream(pkg, j["seed"], j["first"], j["n"]))
        assert (alone == out[j["name"]]).all()


def test_stream_single_window_launch_across_chunk_three(exe, pkg, consts, mixed, tmp_path):
    j = S.straddle_job(consts["STREAM_CHUNK"])
    got = stream_launch(exe, pkg, consts, [j], tmp_path, "window", mode=2)[j["name"]]
    S.assert_stream_equal("launch_glibc_stream, straddle", got, S.reference_stream(pkg, j["seed"], j["first"], j["n"]))
    assert (got == mixed[1][j["name"]]).all()  # the same job among the others, through the jobs kernel


def test_stream_windows_past_2_to_the_32_continue_each_other(exe, pkg, consts, tmp_path):
    jobs = S.overlap_jobs(consts["STREAM_CHUNK"])
    out = stream_launch(exe, pkg, consts, jobs, tmp_path, "overlap")
    S.check_overlaps(pkg, out, consts["STREAM_CHUNK"])


# ---- activeUE ----
@pytest.fixture(scope="module")
def crafted(exe, host, consts, tmp_path_factory):
    A = S.crafted_cases(host)
    return A, S.host_reference(host, A), act_launch(exe, A, tmp_path_factory.mktemp("crafted"), "crafted")


@pytest.fixture(scope="module")
def background(exe, host, consts, tmp_path_factory):
    A = S.random_cases(host)
    return A, S.host_reference(host, A), act_launch(exe, A, tmp_path_factory.mktemp("random"), "random")


def _report(A, got, figures):
    """The figures tests/tools/HARNESS.md records (pytest -s shows them)."""
    print("figures:", figures)
    must = [k for k in range(len(A)) if A.expect.get(A.name[k], {}).get("kind") == "must"]
    if must:
        print("must-flag cases flagged:", int(got["flag"][must].sum()), "of", len(must))


def test_active_ue_on_crafted_draws(crafted, consts):
    A, ref, got = crafted
    figures = S.verify_act(A, ref, got, consts)
    _report(A, got, figures)


def test_active_ue_on_random_draws(background, consts):
    A, ref, got = background
    figures = S.verify_act(A, ref, got, consts, flag_cap_over=("random",))
    _report(A, got, figures)


def test_active_ue_flags_few_of_the_near_misses_and_random_ues(crafted, background, consts):
    counts = [S.capped_counts(A, got) for A, ref, got in (crafted, background)]
    print("(cases, flagged) among the near misses and the random UEs:", counts)
    S.assert_flag_cap(*counts)
