"""tests/tools/stream_act_cases.py and tests/tools/gpu_stream_act_harness.hip without a GPU: the harness compiles for gfx950 and carries the constants the
generator assumes; the host's jump-ahead prach_internal_glibc_seeds (matrix powers, A^chunk, offsets up to 2^40) against a numpy statement of the
recurrence and against the sequential generator; the job tables and the activeUE case groups contain what they are there for according to the host
function — both sides of every edge, the must-flag and near-miss counts per quantity of tests/golden/act_boundaries.json under THIS machine's libm — and the
flag cap of the GPU test holds for the host's classification alone.  tests/test_gpu_stream_act_synthetic.py runs the same cases on the device."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import stream_act_cases as S  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return S.build_harness(tmp_path_factory.mktemp("stream_act_harness"))  # compiles for gfx950


@pytest.fixture(scope="module")
def consts(exe):
    return S.harness_constants(exe)


@pytest.fixture(scope="module")
def host(pkg):
    return S.Host(pkg)


@pytest.fixture(scope="module")
def crafted(host):
    A = S.crafted_cases(host)
    return A, S.host_reference(host, A)


@pytest.fixture(scope="module")
def background(host):
    A = S.random_cases(host)
    return A, S.host_reference(host, A)


def test_harness_carries_the_constants_the_generator_assumes(consts):
    c = consts
    assert c["STREAM_CHUNK"] == 31 * 2048 and c["STREAM_CHUNK"] % 31 == 0
    assert c["ACT_BAND"] == 64 == S.load_boundaries()["act_band"] and c["ACT_GAIN_ULP_ASSERTED"] == 32 and c["NOMA_ACT_FLAG_CAP"] == 8192
    assert c["STREAM_GUARD_WORDS"] >= 64 and c["STREAM_JOB_BYTES"] == 24 and c["SA_ACT_WORDS"] == 10 and c["SA_THREADS"] % 64 == 0
    assert S.PAD_DRAW == 2147483647 // 3


# ---- prach_internal_glibc_seeds ----
def test_roll31_is_the_recurrence():
    rng = np.random.default_rng(5)
    w = rng.integers(0, 2**32, size=31, dtype=np.uint64)
    r = w.tolist()
    for _ in range(31):
        r.append((r[-31] + r[-3]) % 2**32)
    assert S.roll31(w).tolist() == r[31:]


@pytest.mark.parametrize("chunk", [31, 62, 1000 * 31, 63488])
def test_glibc_seeds_windows_against_the_recurrence_and_the_sequential_generator(pkg, consts, chunk):
    assert consts["STREAM_CHUNK"] == 63488
    seeds = S.seeds_fn(pkg)
    nchunks = 9
    for k, first in enumerate((0, 1, 30, 31, 343, 12_345, 40_000_000)):
        seed = S.STREAM_SEEDS[k % len(S.STREAM_SEEDS)]
        W = seeds(seed, first, nchunks, chunk)
        ref = pkg.glibc_stream(seed & 0xFFFFFFFF, first, nchunks * chunk + 62).astype(np.int64)
        if first + 341 <= S.LIBC_PREFIX:
            assert (ref[:341] == S.libc_prefix(seed)[first:first + 341]).all()  # libc's own rand()
        # every window, rolled forward two blocks at once, gives the 62 values behind first + c chunk
        w = W.astype(np.uint64)
        for b in range(2):
            w = S.roll31(w)
            for c in range(nchunks):
                assert ((w[c] >> 1).astype(np.int64) == ref[c * chunk + 31 * b:c * chunk + 31 * b + 31]).all(), (chunk, first, c, b)
        # window 0 rolled through the first chunks reproduces the stream, and arrives at the later windows
        n = min(nchunks * chunk, 70_000)
        assert (S.roll_stream(W[0], n) == ref[:n]).all(), (chunk, first)
        w = W[0].astype(np.uint64)
        for c in range(1, min(nchunks, 70_000 // chunk + 1)):
            for _ in range(chunk // 31):
                w = S.roll31(w)
            assert (w == W[c]).all(), (chunk, first, c)
        # window c equals a fresh call at first + c chunk
        for c in (1, 4, nchunks - 1):
            assert (seeds(seed, first + c * chunk, 1, chunk)[0] == W[c]).all(), (chunk, first, c)
            assert (seeds(seed, first + c * chunk, 1, 31)[0] == W[c]).all()  # (whatever the chunk of that call)


def test_glibc_seeds_overlap_identities_past_2_to_the_32(pkg, consts):
    seeds, chunk = S.seeds_fn(pkg), consts["STREAM_CHUNK"]
    for k, F in enumerate(S.BIG_OFFSETS):
        seed = S.STREAM_SEEDS[2 + k]
        b = S.roll_stream(seeds(seed, F, 1, chunk)[0], S.OVERLAP_B)
        a = S.roll_stream(seeds(seed, F - S.OVERLAP_BACK, 1, chunk)[0], S.OVERLAP_A)
        assert (a[S.OVERLAP_BACK:] == b).all(), F
        W = seeds(seed, F - 2 * chunk, 3, chunk)  # A^chunk twice from F - 2 chunks is the jump to F, and 4096 blocks of the recurrence
        assert (W[2] == seeds(seed, F, 1, chunk)[0]).all(), F
        w = W[0].astype(np.uint64)
        for c in (1, 2):
            for _ in range(chunk // 31):
                w = S.roll31(w)
            assert (w == W[c]).all(), (F, c)


def test_stream_jobs_contain_what_they_are_there_for(consts):
    chunk = consts["STREAM_CHUNK"]
    jobs = S.mixed_jobs(chunk)
    ns = [j["n"] for j in jobs]
    assert sorted(ns) == sorted(S.stream_lengths(chunk) + [70_000]) and {j["seed"] for j in jobs} == set(S.STREAM_SEEDS)
    assert S.stream_lengths(chunk) == [1, 2, 30, 31, 32, 61, 62, 63, chunk - 1, chunk, chunk + 1, 4 * chunk, 4 * chunk + 1, 9 * chunk - 17]
    assert ns.index(max(ns)) not in (0, len(ns) - 1) and ns != sorted(ns)
    assert any(j["first"] == 3 * chunk - 5 for j in jobs) and len({j["first"] for j in jobs}) >= 6
    assert sum(ns) < 1_400_000  # (the issue's list of lengths: 20 chunks and a little)
    ov = S.overlap_jobs(chunk)
    assert {j["F"] for j in ov} == {2**32 - 1000, 2**32, 2**40 + 12_345, 40_000_000} and sum(j["n"] for j in ov) < 10**6
    for j in ov:
        assert j["first"] in (j["F"] - 70_000, j["F"], j["F"] - 2 * chunk)


# ---- activeUE ----
def test_every_expectation_with_a_host_reference_is_the_hosts(crafted):
    A, ref = crafted
    assert (ref["rc"][A.has_host] == 0).all()
    for name, e in A.expect.items():
        k = A.index[name]
        if A.has_host[k]:
            for fld in ("used", "sec"):
                if fld in e:
                    assert ref[fld][k] == e[fld], (name, fld, int(ref[fld][k]), e[fld])


def test_sector_edges_hold_both_sides_of_all_five_boundaries(crafted, host):
    A, ref = crafted
    edges = S.sector_edges(host)
    assert edges == sorted(edges) and len(set(edges)) == 5
    for s in range(1, 6):
        for side in (0, 1):
            k = [A.index[n] for n, e in A.expect.items() if e.get("edge") == s and e.get("side") == side]
            assert len(k) == 64 and (ref["sec"][k] == s - 1 + side).all(), (s, side)
    assert ref["sec"][A.index[f"sector_draw{2**30}"]] == 3 and host.one([5, edges[2] - 1, S.RACC, S.GACC], 400.0)[2] == 2  # angle == pi: the float comparison
    # ((float)(2^30 - 1) is 2^30: the draw before 2^30 is in sector 3 as well, the last one of sector 2 is edges[2] - 1)
    assert ref["sec"][A.index["sector_draw0"]] == 0 and ref["sec"][A.index[f"sector_draw{S.DMAX}"]] == 5


def test_radius_and_gain_edges_hold_both_sides(crafted):
    A, ref = crafted
    for R in S.RADII:
        k = np.asarray([i for i, n in enumerate(A.name) if n.startswith((f"radius{R:g}+", f"radius{R:g}-"))])
        assert len(k) == 16 and (ref["used"][k[:8]] == 5).all() and (ref["used"][k[8:]] == 4).all(), R
        assert ref["used"][A.index[f"radius{R:g}_draw0"]] == 5
    assert S.GAIN_PAIRS >= 32
    for p in range(S.GAIN_PAIRS):
        k = np.asarray([i for i, n in enumerate(A.name) if n.startswith(f"gain{p}_")])
        assert len(k) == 8 and (ref["used"][k[:4]] == 4).all() and (ref["used"][k[4:]] == 5).all(), p
        assert (ref["gain"][k] >= 1e-7).all() and (ref["gain"][k[:4]] < 1.0001e-7).all()  # the accept side's gain is the threshold's neighbour
    for R in (36.0, 400.0, 2000.0):
        assert np.isinf(ref["gain"][A.index[f"gain_draw0_{R:g}"]]) and ref["used"][A.index[f"gain_ten_rejected_{R:g}"]] == 14


def test_caps_and_budgets_are_sized_as_stated(crafted, host):
    A, ref = crafted
    for name in ("cap_radius", "cap_gain"):
        k = A.index[name]
        assert A.budget[k] >= A.expect[name]["used"] + 3 and not A.has_host[k]  # `oob` stays 0
    for name, e in A.expect.items():
        if e.get("extended"):  # what the device takes past the list is what the host takes from PAD_DRAW
            d = A.draws(A.index[name]).tolist()
            assert host.one(d, 400.0)[0] != 0  # the list alone ends inside a loop (PRACH_ERR_STREAM)
            assert host.one(d + [S.PAD_DRAW] * 8, 400.0)[5] == e["used"] > len(d), name
    f = np.float32
    assert f(36.0) * np.sqrt(np.float64(f(f(S.PAD_DRAW) * f(2.0**-31)))) < 35.0  # every draw past the list is rejected at cellRadius 36


def test_float_boundary_cases_classify_as_stated_under_this_libm(crafted, host, consts):
    A, ref = crafted
    B = S.load_boundaries()
    band = consts["ACT_BAND"]
    count = {}
    for c in B["cases"]:
        px, py, pld, r = host.quantities(c["angle"], c["rdraw"], B["radius"])
        dist = dict(zip(("px", "py", "pld"), (int(S.boundary_distance(v)) for v in (px, py, pld))))
        assert r > 35.0
        others = [dist[q] for q in dist if q != c["q"]]
        if c["kind"] == "must":
            assert 2 * dist[c["q"]] <= band and min(others) >= 4 * band, (c, dist)  # this quantity alone, within ACT_BAND / 2
        else:
            assert 4 * band <= dist[c["q"]] <= 8 * band and min(others) >= 4 * band, (c, dist)  # nothing within ACT_BAND of a boundary
        count[(c["q"], c["kind"])] = count.get((c["q"], c["kind"]), 0) + 1
        count[(c["q"], c["kind"], c["side"])] = count.get((c["q"], c["kind"], c["side"]), 0) + 1
    for q in ("px", "py", "pld"):
        assert count[(q, "must")] >= 8 and count[(q, "near")] >= 8, count
    for q in ("px", "py"):  # dropped bits above and below the midpoint: a mask one bit short sees only the ones below
        assert count[(q, "must", 1)] >= 3 and count[(q, "must", -1)] >= 3, count
    k = np.flatnonzero(A.group == "float_boundaries")
    assert len(k) == len(B["cases"]) and (ref["used"][k] == 4).all()


def test_flag_cap_holds_for_the_hosts_classification_alone(crafted, background, host, consts):
    band = consts["ACT_BAND"]
    n = flagged = 0
    for A, ref in (crafted, background):
        dist = S.host_flag_distance(host, A)
        m = np.isin(A.group, ["random"]) | np.asarray([A.expect.get(x, {}).get("kind") == "near" for x in A.name])
        near = np.asarray([A.expect.get(x, {}).get("kind") == "near" for x in A.name])
        assert (dist[near] > band).all()  # none of the near misses lies within ACT_BAND of a boundary
        must = np.asarray([A.expect.get(x, {}).get("kind") == "must" for x in A.name])
        assert (2 * dist[must] <= band).all()
        n += int(m.sum())
        flagged += int((m & (dist <= band)).sum())
    print(f"{flagged} of {n} near-miss and random cases within ACT_BAND of a boundary by the host's libm (expected for the random ones: {n * 3 * (2 * band + 1) / 2**29:.2f})")
    assert n >= S.RANDOM_UES and flagged <= n // S.FLAG_CAP_PER


def test_random_background(background):
    A, ref = background
    assert len(A) == S.RANDOM_UES == 200_000 and (ref["rc"] == 0).all()
    for R, lo, hi in ((36.0, 15, 30), (400.0, 4, 4.2), (2000.0, 4, 4.5)):
        m = A.radius == np.float32(R)
        assert m.sum() >= S.RANDOM_UES // 3 and lo < ref["used"][m].mean() < hi, (R, ref["used"][m].mean())
    assert (A.budget >= ref["used"]).all() and len(A.pool) < 3_000_000
    assert set(np.unique(ref["sec"]).tolist()) == {0, 1, 2, 3, 4, 5}
