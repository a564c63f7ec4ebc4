"""The device rand() stream generator (csrc/prach_stream.hip, fed by the host's prach_internal_glibc_seeds) and the device activeUE (csrc/prach_noma_act.h)
away from every trial: a deterministic generator of cases no Monte-Carlo trial produces, their references — libc's own rand(), the host's
prach_noma_activation_stream with the reference's libm, a numpy statement of the lagged-Fibonacci recurrence — and the glue around
tests/tools/gpu_stream_act_harness.hip (case file, result file, one child process per launch).  Shared by tests/test_stream_act_cases_cpu.py,
tests/test_gpu_stream_act_synthetic.py and tests/golden/make_act_boundaries.py.  No GPU here; the constants of the product's headers come from
`gpu_stream_act_harness --constants`, the seed windows from the library's own exported prach_internal_glibc_seeds (the library loads without a device)."""
import ctypes as C
import json
import os

import numpy as np

import harness
from harness import constants as harness_constants  # noqa: F401

MAGIC = 0x53414354
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
HARNESS = "gpu_stream_act_harness.hip"
BOUNDARIES_JSON = os.path.join(ROOT, "tests", "golden", "act_boundaries.json")
PRODUCT_FLAGS = ["-ffp-contract=off"]  # on top of harness.FLAGS
FILL_WORD = 0xA5A5A5A5
DMAX = 2**31 - 1
PAD_DRAW = DMAX // 3      # what draw() returns past the budget (noma_glibc_trial_kernel's convention)
RACC = DMAX               # a radius draw every cell radius accepts: u == 1, r == cellRadius
RGACC = 2126008811        # 0.99 x 2^31: accepted as a radius draw (r = 0.995 cellRadius > 35 from cellRadius 36 on) AND as the gain draw of a UE at r = 35
GACC = 1000               # a gain draw every case here accepts: u = 4.7e-7, -2 ln u = 29, gain >= 29 / (1 + 2000^2)
LIBC_PREFIX = 200_000     # libc's rand() is replayed this far per seed; pkg.glibc_stream (held to libc by tests/test_oracle_rng.py) beyond
ITER_CAP = 4096           # the loop caps of noma_active_ue: `it >= 4096` after the draw, i.e. 4097 draws


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    return harness.build(HARNESS, out_dir, PRODUCT_FLAGS)


def run_harness(exe, case_path, result_path, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    harness.run(exe, [case_path, result_path], timeout)


# ---- the rand() stream ------------------------------------------------------------------------------------------------------------------------------------

def seeds_fn(pkg):
    L = pkg.lib()
    L.prach_internal_glibc_seeds.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.prach_internal_glibc_seeds.restype = None

    def seeds(seed, first, nchunks, chunk):
        out = np.empty((nchunks, 31), dtype=np.uint32)
        L.prach_internal_glibc_seeds(seed & 0xFFFFFFFF, first, nchunks, chunk, out.ctypes.data)
        return out
    return seeds


def roll31(w):
    """The window(s) w[..., 31] = r[m-30 .. m] one block on: r[m+1 .. m+31], by r[i] = r[i-31] + r[i-3] mod 2^32 — y[j] = w[j] + (w[28+j] if j < 3 else y[j-3])."""
    w = np.asarray(w, dtype=np.uint64)
    y = np.empty_like(w)
    for q in range(3):
        y[..., q::3] = np.cumsum(w[..., q::3], axis=-1) + w[..., 28 + q:29 + q]
    return y & 0xFFFFFFFF


def roll_stream(w, n):
    """The n rand() values behind one window, by the recurrence alone (numpy)."""
    out = np.empty((n + 30) // 31 * 31, dtype=np.int64)
    w = np.asarray(w, dtype=np.uint64)
    for b in range(len(out) // 31):
        w = roll31(w)
        out[31 * b:31 * b + 31] = w >> 1
    return out[:n]


_libc_prefix = {}


def libc_prefix(seed):
    if seed not in _libc_prefix:
        libc = C.CDLL("libc.so.6")
        libc.srand(C.c_uint(seed & 0xFFFFFFFF))
        _libc_prefix[seed] = np.fromiter((libc.rand() for _ in range(LIBC_PREFIX)), dtype=np.int64, count=LIBC_PREFIX)
    return _libc_prefix[seed]


def reference_stream(pkg, seed, first, n):
    """rand() values first .. first + n - 1 after srand(seed): libc itself below LIBC_PREFIX, the host's sequential generator beyond."""
    parts = []
    if first < LIBC_PREFIX:
        parts.append(libc_prefix(seed)[first:min(first + n, LIBC_PREFIX)])
    lo = max(first, LIBC_PREFIX)
    if first + n > lo:
        parts.append(pkg.glibc_stream(seed & 0xFFFFFFFF, lo, first + n - lo).astype(np.int64))
    return np.concatenate(parts)


STREAM_SEEDS = (0, 1, 7, 2022, 2**31 - 1, 2**32 - 1)
STREAM_FIRSTS = (0, 1, 30, 31, 343, 12_345)
BIG_OFFSETS = (2**32 - 1000, 2**32, 2**40 + 12_345)
ANCHOR_OFFSET = 40_000_000
OVERLAP_BACK, OVERLAP_A, OVERLAP_B = 70_000, 71_000, 1000


def stream_lengths(chunk):
    return [1, 2, 30, 31, 32, 61, 62, 63, chunk - 1, chunk, chunk + 1, 4 * chunk, 4 * chunk + 1, 9 * chunk - 17]


def straddle_job(chunk):
    return dict(name="straddle", seed=2022, first=3 * chunk - 5, n=70_000)  # tests/test_gpu_parity.py::test_device_glibc_stream_matches_libc's


def mixed_jobs(chunk):
    """Every length of the list, each with a seed and an offset of its own, and the straddle; shuffled (fixed), the longest neither first nor last."""
    jobs = [dict(name=f"n{n}", seed=STREAM_SEEDS[k % 6], first=STREAM_FIRSTS[(5 * k + 1) % 6], n=n) for k, n in enumerate(stream_lengths(chunk))]
    jobs.append(straddle_job(chunk))
    order = np.random.default_rng(20240607).permutation(len(jobs))
    jobs = [jobs[i] for i in order]
    longest = max(range(len(jobs)), key=lambda j: jobs[j]["n"])
    if longest in (0, len(jobs) - 1):
        jobs[longest], jobs[len(jobs) // 2] = jobs[len(jobs) // 2], jobs[longest]
    return jobs


def longest_job(chunk):
    return next(j for j in mixed_jobs(chunk) if j["n"] == 9 * chunk - 17)


def overlap_jobs(chunk):
    """Per offset F: A = [F - 70 000, +71 000), B = [F, +1000), C = [F - 2 chunks, F + 1000).  A's and C's tails are B.  F = 40 000 000 is replayable."""
    jobs = []
    for k, F in enumerate(BIG_OFFSETS + (ANCHOR_OFFSET,)):
        seed = (2022, 2**32 - 1, 7, 3)[k]
        jobs += [dict(name=f"A@{F}", seed=seed, first=F - OVERLAP_BACK, n=OVERLAP_A, F=F), dict(name=f"B@{F}", seed=seed, first=F, n=OVERLAP_B, F=F),
                 dict(name=f"C@{F}", seed=seed, first=F - 2 * chunk, n=2 * chunk + OVERLAP_B, F=F)]
    return jobs


def write_stream_case(path, jobs, seeds, chunk, mode=1):
    h = np.zeros(16, dtype="<u4")
    h[:3] = [MAGIC, mode, len(jobs)]
    tab = np.zeros((len(jobs), 4), dtype="<u4")
    wins = []
    for k, j in enumerate(jobs):
        nch = (j["n"] + chunk - 1) // chunk
        tab[k] = [j["n"] & 0xFFFFFFFF, j["n"] >> 32, nch, 0]
        wins.append(seeds(j["seed"], j["first"], nch, chunk))
    with open(path, "wb") as f:
        f.write(h.tobytes())
        f.write(tab.tobytes())
        for w in wins:
            f.write(np.ascontiguousarray(w, dtype="<u4").tobytes())
    return wins


def read_stream_result(path, jobs, wins, consts, mode=1):
    """{job name: its output words}; asserts on the way that the windows came back as sent and that every word of the arena outside the job table, the
    windows and the outputs — the guard words behind every output, the gaps between the arrays — still holds the fill pattern."""
    r = np.fromfile(path, dtype="<u4")
    n = len(jobs)
    assert r[:3].tolist() == [MAGIC, mode, n], r[:8].tolist()
    words, jt_off, jt_len = int(r[3]), int(r[4]), int(r[5])
    assert jt_len * 4 == consts["STREAM_JOB_BYTES"] * n
    layout = r[8:8 + 2 * n].reshape(n, 2).astype(np.int64)
    arena = r[8 + 2 * n:]
    assert len(arena) == words
    free = np.ones(words, dtype=bool)
    free[jt_off:jt_off + jt_len] = False
    out = {}
    for j, w, (so, oo) in zip(jobs, wins, layout.tolist()):
        assert so % 64 == 0 and oo % 64 == 0  # 256-byte alignment
        assert free[so:so + w.size].all() and free[oo:oo + j["n"] + consts["STREAM_GUARD_WORDS"]].all(), f"{j['name']}: arrays overlap"
        assert (arena[so:so + w.size] == w.reshape(-1)).all(), f"{j['name']}: the seed windows were written to"
        free[so:so + w.size] = False
        free[oo:oo + j["n"]] = False
        guard = arena[oo + j["n"]:oo + j["n"] + consts["STREAM_GUARD_WORDS"]]
        assert (guard == FILL_WORD).all(), f"{j['name']} (n = {j['n']}): guard words {np.flatnonzero(guard != FILL_WORD)[:8].tolist()} behind the output were written"
        out[j["name"]] = arena[oo:oo + j["n"]].astype(np.int64)
    bad = np.flatnonzero(free & (arena != FILL_WORD))
    assert bad.size == 0, f"{bad.size} words outside every array were written, first at {bad[:8].tolist()} (layout {layout.tolist()})"
    return out


def assert_stream_equal(name, got, ref):
    bad = np.flatnonzero(got != ref)
    assert len(got) == len(ref) and bad.size == 0, f"{name}: {bad.size} of {len(ref)} values differ, first at {bad[:6].tolist()}: {got[bad[:3]].tolist()} for {ref[bad[:3]].tolist()}"


def check_overlaps(pkg, out, chunk):
    for F in BIG_OFFSETS + (ANCHOR_OFFSET,):
        a, b, c = out[f"A@{F}"], out[f"B@{F}"], out[f"C@{F}"]
        assert_stream_equal(f"A@{F} tail against B", a[OVERLAP_BACK:], b)
        assert_stream_equal(f"C@{F} tail against B", c[2 * chunk:], b)
        assert_stream_equal(f"A@{F} against C where they overlap", a, c[2 * chunk - OVERLAP_BACK:2 * chunk - OVERLAP_BACK + OVERLAP_A])
    F = ANCHOR_OFFSET
    for j in overlap_jobs(chunk):
        if j["F"] == F:
            assert_stream_equal(j["name"], out[j["name"]], pkg.glibc_stream(j["seed"], j["first"], j["n"]).astype(np.int64))


# ---- activeUE: the host side ------------------------------------------------------------------------------------------------------------------------------

class Host:
    """prach_noma_activation_stream (csrc/prach_host.c, the reference's libm) on draw lists, and the C library's cos / sin / sqrt / pow for the three
    values the reference rounds to float."""

    def __init__(self, pkg):
        self.pkg = pkg
        L = pkg.lib()
        self.fn = L.prach_noma_activation_stream
        self.fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.fn.restype = C.c_int
        m = C.CDLL("libm.so.6")
        for f in ("cos", "sin", "sqrt"):
            getattr(m, f).argtypes = [C.c_double]
            getattr(m, f).restype = C.c_double
        m.pow.argtypes = [C.c_double, C.c_double]
        m.pow.restype = C.c_double
        self.m = m
        self._cfg = {}

    def cfg(self, radius, nP):
        key = (float(np.float32(radius)), int(nP))
        if key not in self._cfg:
            self._cfg[key] = self.pkg.make_cfg(1, variant=self.pkg.VARIANT_NOMA_C, rng_mode=self.pkg.RNG_GLIBC, cellRadius=key[0], nPreamble=key[1])
        return self._cfg[key]

    def walk(self, pool, off, budget, radius, nP):
        """The host function on pool[off[k] : off[k] + budget[k]] for every k: rc, pre, sec, gain, lgain, used (used = 0 where rc != 0)."""
        pool = np.ascontiguousarray(pool, dtype=np.int32)
        n = len(off)
        rc, pre, sec, used = (np.zeros(n, dtype=np.int32) for _ in range(4))
        gain, lgain = np.zeros(n), np.zeros(n)
        pos = C.c_uint64(0)
        pp, base = C.addressof(pos), pool.ctypes.data
        ap, asec, ag, al = pre.ctypes.data, sec.ctypes.data, gain.ctypes.data, lgain.ctypes.data
        for k in range(n):
            assert 0 <= off[k] and off[k] + budget[k] <= len(pool)
            pos.value = 0
            rc[k] = self.fn(C.addressof(self.cfg(radius[k], nP[k])), base + 4 * int(off[k]), pp, int(budget[k]), ap + 4 * k, asec + 4 * k, ag + 8 * k, al + 8 * k)
            used[k] = pos.value if rc[k] == 0 else 0
        return rc, pre, sec, gain, lgain, used

    def one(self, draws, radius, nP=54):
        rc, pre, sec, gain, lgain, used = self.walk(np.asarray(draws, dtype=np.int32), [0], [len(draws)], [radius], [nP])
        return int(rc[0]), int(pre[0]), int(sec[0]), float(gain[0]), float(lgain[0]), int(used[0])

    def quantities(self, adraw, rdraw, radius):
        """r cos(angle), r sin(angle), sqrt(1 + env^2) as prach_noma_activation_stream forms them (doubles, before they are rounded to float), with the C
        library's cos, sin, sqrt and pow."""
        f = np.float32
        a = f(f(f(f(adraw) * f(2.0**-31)) * f(2)) * f(3.14))
        r = f(float(f(radius)) * self.m.sqrt(float(f(f(rdraw) * f(2.0**-31)))))
        px, py = float(r) * self.m.cos(float(a)), float(r) * self.m.sin(float(a))
        x, y = f(px), f(py)
        env = self.m.sqrt(float(f(f(x * x) + f(y * y))))
        pld = self.m.sqrt(1 + self.m.pow(env, 2.0))
        return px, py, pld, float(r)


def boundary_distance(p):
    """|the 29 bits a float drops - their midpoint 2^28|: how many double ulps p lies from the nearest float rounding boundary."""
    bits = np.asarray(p, dtype=np.float64).view(np.int64)
    return np.abs((bits & ((1 << 29) - 1)) - (1 << 28))


def quantities_np(adraw, rdraw, radius):
    """The same three values with numpy's cos / sin (a PREFILTER only: numpy's may differ from the C library's in the last bits), and r."""
    f = np.float32
    a = (f(np.asarray(adraw)) * f(2.0**-31) * f(2) * f(3.14)).astype(np.float64)
    r = (np.float64(f(radius)) * np.sqrt((f(np.asarray(rdraw)) * f(2.0**-31)).astype(np.float64))).astype(f)
    px, py = r.astype(np.float64) * np.cos(a), r.astype(np.float64) * np.sin(a)
    x, y = px.astype(f), py.astype(f)
    env = np.sqrt((x * x + y * y).astype(np.float64))
    return px, py, np.sqrt(1 + env * env), r


def bisect(lo, hi, pred):
    """The smallest d in (lo, hi] with pred(d), given not pred(lo), pred(hi) and a monotone pred."""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


# ---- activeUE: the cases ----------------------------------------------------------------------------------------------------------------------------------
RADII = (36.0, 40.0, 60.0, 400.0, 1500.0, 2000.0)
RANDOM_RADII = (36.0, 400.0, 2000.0)
RANDOM_UES = 200_000
FLAG_CAP_PER = 100_000  # at most 1 in 10^5 of the near-miss and random cases may be flagged
GAIN_PAIRS = 36
SIDE = 64


class ActCases:
    def __init__(self):
        self.name, self.group, self.off, self.budget, self.radius, self.nP, self.has_host = [], [], [], [], [], [], []
        self.chunks, self.at = [], 0
        self.expect = {}  # name -> dict of expectations that do not come from the host function

    def add(self, group, name, draws, radius, nP=54, budget=None, has_host=True, **expect):
        draws = np.asarray(draws, dtype=np.int64)
        assert draws.min() >= 0 and draws.max() <= DMAX
        self.add_window(group, name, self.at, len(draws) if budget is None else budget, radius, nP, has_host, **expect)
        self.chunks.append(draws.astype(np.int32))
        self.at += len(draws)

    def add_window(self, group, name, off, budget, radius, nP=54, has_host=True, **expect):
        self.name.append(name); self.group.append(group); self.off.append(off); self.budget.append(budget)
        self.radius.append(radius); self.nP.append(nP); self.has_host.append(has_host)
        if expect:
            self.expect[name] = expect

    def finish(self):
        self.pool = np.concatenate(self.chunks)
        assert len(self.pool) == self.at
        for k in ("off", "budget", "nP"):
            setattr(self, k, np.asarray(getattr(self, k), dtype=np.int64))
        self.radius = np.asarray(self.radius, dtype=np.float32)
        self.has_host = np.asarray(self.has_host, dtype=bool)
        self.group = np.asarray(self.group)
        self.index = {n: k for k, n in enumerate(self.name)}
        assert len(self.index) == len(self.name)
        assert (self.off + self.budget <= len(self.pool)).all()
        return self

    def __len__(self):
        return len(self.name)

    def draws(self, k):
        return self.pool[self.off[k]:self.off[k] + self.budget[k]]


def sector_edges(H, radius=400.0):
    """The five draws at which the host's sector changes: edge[s - 1] = the smallest angle draw in sector >= s."""
    return [bisect(0, DMAX, lambda d, s=s: H.one([5, d, RACC, GACC], radius)[2] >= s) for s in range(1, 6)]


def radius_edge(H, radius):
    """The smallest radius draw the host accepts: RGACC behind it is then the gain draw (4 draws used), behind a rejected one the next radius draw (5)."""
    hi = min(DMAX, int(1.02 * (35.0 / radius) ** 2 * 2**31) + 1000)  # (r = 35.3: RGACC is a gain draw this close to 35 only)
    return bisect(0, hi, lambda d: H.one([5, 12_345, d, RGACC, GACC, GACC], radius)[5] == 4)


def gain_edge(H, adraw, rdraw, radius):
    """The smallest gain draw the host rejects (ch_g < 1e-7: a fifth draw)."""
    return bisect(0, DMAX, lambda g: H.one([5, adraw, rdraw, g, GACC], radius)[5] == 5)


def load_boundaries():
    with open(BOUNDARIES_JSON) as f:
        return json.load(f)


def crafted_cases(H):
    A = ActCases()
    # sector_edges
    for s, e in enumerate(sector_edges(H), start=1):
        for d in range(e - SIDE, e + SIDE):
            A.add("sector_edges", f"sector{s}{d - e:+d}", [7 * s + 1, d, RACC, GACC], 400.0, side=int(d >= e), edge=s)
    for d, sec in ((2**30, 3), (2**30 - 1, None), (0, 0), (DMAX, 5)):
        A.add("sector_edges", f"sector_draw{d}", [53, d, RACC, GACC], 400.0, **({} if sec is None else dict(sec=sec)))
    # radius_edge
    for R in RADII:
        e = radius_edge(H, R)
        for d in range(e - 8, e + 8):
            A.add("radius_edge", f"radius{R:g}{d - e:+d}", [9, 987_654_321, d, RGACC, GACC, GACC], R, used=4 if d >= e else 5)
        A.add("radius_edge", f"radius{R:g}_draw0", [9, 987_654_321, 0, RGACC, GACC, GACC], R, used=5)
    # gain_threshold
    rng = np.random.default_rng(1857)
    for k in range(GAIN_PAIRS):
        R = RADII[k % len(RADII)]
        re = radius_edge(H, R)
        rd, ad = int(rng.integers(re, DMAX + 1)), int(rng.integers(0, DMAX + 1))
        e = gain_edge(H, ad, rd, R)
        for g in range(e - 4, e + 4):
            A.add("gain_threshold", f"gain{k}_{R:g}{g - e:+d}", [k, ad, rd, g, GACC], R, used=5 if g >= e else 4)
    # gain_extremes
    for R in (36.0, 400.0, 2000.0):
        A.add("gain_extremes", f"gain_draw0_{R:g}", [1, 555_555_555, RACC, 0, GACC], R, used=4, flag=1, infinite=True)
        A.add("gain_extremes", f"gain_drawmax_{R:g}", [1, 555_555_555, RACC, DMAX, GACC], R, used=5)
        A.add("gain_extremes", f"gain_ten_rejected_{R:g}", [1, 555_555_555, RACC] + [DMAX - j for j in range(10)] + [GACC], R, used=14)
    # iteration_caps: no host comparison (the host would go on); 4097 draws of the capped loop, then the device ends
    rej_r = [1000 * j for j in range(4200)]  # u < 0.002: r < 0.045 cellRadius = 18 at cellRadius 400
    A.add("iteration_caps", "cap_radius", [3, 1_000_000_000] + rej_r + [GACC] * 4, 400.0, has_host=False, flag=1, oob=0, used=2 + ITER_CAP + 1 + 1)
    A.add("iteration_caps", "cap_gain", [3, 1_000_000_000, RACC] + [DMAX - j for j in range(4200)] + [GACC] * 4, 400.0, has_host=False, flag=1, oob=0,
          used=3 + ITER_CAP + 1)
    # budget: the list ends inside a loop; past it draw() returns PAD_DRAW (r = 0.577 cellRadius, a gain of 2.2 / pathloss^2: both accepted at 400)
    A.add("budget", "budget_in_radius_loop", [3, 77, 1000, 2000], 400.0, has_host=False, oob=1, used=4 + 2, extended=True)
    A.add("budget", "budget_in_gain_loop", [3, 77, RACC, DMAX, DMAX - 1], 400.0, has_host=False, oob=1, used=5 + 1, extended=True)
    A.add("budget", "budget_before_the_angle", [3], 400.0, has_host=False, oob=1, used=1 + 3, extended=True)
    # (cellRadius 36: 0.577 x 36 < 35, every draw past the list is rejected until the cap ends the loop)
    A.add("budget", "budget_in_radius_loop_r36", [3, 77, 1000, 2000], 36.0, has_host=False, oob=1, flag=1, used=2 + ITER_CAP + 1 + 1)
    # float_boundaries
    B = load_boundaries()
    for k, c in enumerate(B["cases"]):
        A.add("float_boundaries", f"{c['kind']}_{c['q']}_{k}", [11, c["angle"], c["rdraw"], GACC], B["radius"], kind=c["kind"], q=c["q"])
    return A.finish()


def random_cases(H):
    """RANDOM_UES UEs of uniform 31-bit draws, a third at each radius; like the arrivals of a glibc-mode trial every UE starts where the host says the one
    before it ended (the budget a few draws more than the host takes, so a device that takes more does not run into `oob` at once)."""
    A = ActCases()
    rng = np.random.default_rng(424242)
    for R, per in zip(RANDOM_RADII, (26, 5, 5)):
        n = RANDOM_UES // len(RANDOM_RADII) + (1 if R == RANDOM_RADII[0] else 0) * (RANDOM_UES % len(RANDOM_RADII))
        pool = rng.integers(0, 2**31, size=n * per + 64, dtype=np.int64).astype(np.int32)
        base, at = A.at, 0
        cfg = H.cfg(R, 54)
        pos = C.c_uint64(0)
        o = (C.c_int32 * 2)()
        g = (C.c_double * 2)()
        for k in range(n):
            at = pos.value
            rc = H.fn(C.addressof(cfg), pool.ctypes.data, C.addressof(pos), len(pool), C.addressof(o), C.addressof(o) + 4, C.addressof(g), C.addressof(g) + 8)
            assert rc == 0, "the random pool is too short"
            A.add_window("random", f"random{R:g}_{k}", base + at, min(pos.value - at + 8, len(pool) - at), R)
        A.chunks.append(pool)
        A.at += len(pool)
    return A.finish()


def write_act_case(path, A):
    h = np.zeros(16, dtype="<u4")
    h[:4] = [MAGIC, 3, len(A), len(A.pool)]
    tab = np.zeros((len(A), 4), dtype="<u4")
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3] = A.off, A.budget, A.radius.view(np.uint32), A.nP
    with open(path, "wb") as f:
        f.write(h.tobytes())
        f.write(tab.tobytes())
        f.write(A.pool.astype("<i4").tobytes())


def read_act_result(path, n):
    r = np.fromfile(path, dtype="<u4")
    assert r[:3].tolist() == [MAGIC, 3, n] and len(r) == 8 + 10 * n, r[:8].tolist()
    w = r[8:].reshape(n, 10).astype(np.int64)
    gb, lb = w[:, 2] | w[:, 3] << 32, w[:, 4] | w[:, 5] << 32
    assert (w[:, 9] == 0).all() and (w[:, 6] <= 1).all() and (w[:, 8] <= 1).all()
    return dict(pre=w[:, 0], sec=w[:, 1], gain_bits=gb, gain=gb.view(np.float64), lgain=lb.view(np.float64), flag=w[:, 6].astype(bool), used=w[:, 7], oob=w[:, 8].astype(bool))


def host_reference(H, A):
    """rc, pre, sec, gain, lgain, used of the host function for the cases that have one (rc = -1 for the others)."""
    k = np.flatnonzero(A.has_host)
    rc, pre, sec, gain, lgain, used = (np.zeros(len(A), dtype=t) for t in (np.int32, np.int32, np.int32, np.float64, np.float64, np.int32))
    rc[:] = -1
    rc[k], pre[k], sec[k], gain[k], lgain[k], used[k] = H.walk(A.pool, A.off[k], A.budget[k], A.radius[k], A.nP[k])
    return dict(rc=rc, pre=pre, sec=sec, gain=gain, lgain=lgain, used=used)


def host_flag_distance(H, A):
    """For every case: the smallest distance (double ulps) of the host's px, py, pld from a float rounding boundary — numpy as a prefilter, the C library's
    cos / sin / sqrt for every case numpy puts within 1024 ulps.  The radius draw is the first one of the case's list the radius loop accepts (2^28 for a
    case without one)."""
    f = np.float32
    dist = np.full(len(A), 2**28, dtype=np.int64)
    for R in np.unique(A.radius):
        u = (A.pool.astype(f) * f(2.0**-31)).astype(np.float64)
        acc = (np.float64(R) * np.sqrt(u)).astype(f).astype(np.float64) > 35.0
        nxt = np.where(acc, np.arange(len(A.pool)), len(A.pool))
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]  # the first accepted draw at or behind each position
        k = np.flatnonzero((A.radius == R) & (A.budget >= 3))
        j = nxt[A.off[k] + 2]
        ok = j < A.off[k] + A.budget[k]
        k, j = k[ok], j[ok]
        px, py, pld, _ = quantities_np(A.pool[A.off[k] + 1], A.pool[j], R)
        d = np.minimum(np.minimum(boundary_distance(px), boundary_distance(py)), boundary_distance(pld))
        for i in np.flatnonzero(d <= 1024):  # (numpy's cos within a few ulp of the C library's: everything closer than this is decided by the latter)
            d[i] = min(int(boundary_distance(q)) for q in H.quantities(int(A.pool[A.off[k[i]] + 1]), int(A.pool[j[i]]), R)[:3])
        dist[k] = d
    return dist


def capped_counts(A, got, over=("random",)):
    """(cases, flagged ones) among the groups `over` and the near misses of float_boundaries."""
    m = np.isin(A.group, list(over)) | np.asarray([A.expect.get(n, {}).get("kind") == "near" for n in A.name])
    return int(m.sum()), int((m & got["flag"]).sum())


def ulp_distance(a_bits, b):
    return np.abs(np.asarray(a_bits, dtype=np.int64) - np.asarray(b, dtype=np.float64).view(np.int64))


def verify_act(A, ref, got, consts, flag_cap_over=()):
    """The assertions on one act launch; returns the figures of the run.  `flag_cap_over`: the groups whose flagged cases count against the 1-in-10^5 cap."""
    figures = {}
    h = A.has_host
    assert (ref["rc"][h] == 0).all(), [A.name[k] for k in np.flatnonzero(h & (ref["rc"] != 0))[:5]]
    names = np.asarray(A.name)

    def first(bad):
        k = np.flatnonzero(bad)[:5]
        return f"{int(bad.sum())} cases, first {names[k].tolist()}: draws {[A.draws(i)[:8].tolist() for i in k[:2]]}"
    assert not got["oob"][h].any(), "a draw past the budget: " + first(h & got["oob"])
    for fld, what in (("pre", "preamble"), ("sec", "sector"), ("used", "draws used")):
        bad = h & (got[fld] != ref[fld])
        assert not bad.any(), f"{what}: {first(bad)}: device {got[fld][bad][:5].tolist()} (flag {got['flag'][bad][:5].tolist()}), host {ref[fld][bad][:5].tolist()}"
    un = h & ~got["flag"]
    assert np.isfinite(ref["gain"][un]).all() and (ref["gain"][un] >= 1e-7).all(), "an unflagged case whose host gain is not finite: " + first(un & ~np.isfinite(ref["gain"]))
    ulp = ulp_distance(got["gain_bits"], ref["gain"])
    bad = un & (ulp > consts["ACT_GAIN_ULP_ASSERTED"])
    assert not bad.any(), f"gain of an unflagged case off by more than {consts['ACT_GAIN_ULP_ASSERTED']} ulp: {first(bad)}: {ulp[bad][:5].tolist()} ulp"
    with np.errstate(invalid="ignore"):
        bad = un & ~(np.abs(got["lgain"] - ref["lgain"]) < 1e-13)
    assert not bad.any(), f"ln gain of an unflagged case: {first(bad)}"
    for g in np.unique(A.group):
        m = un & (A.group == g)
        if m.any():
            figures[f"worst_ulp_{g}"] = int(ulp[m].max())
        figures[f"flagged_{g}"] = int((got["flag"] & (A.group == g)).sum())
        figures[f"cases_{g}"] = int((A.group == g).sum())
    # expectations that are the case's own
    must_unflagged = []
    for name, e in A.expect.items():
        k = A.index[name]
        for fld in ("used", "sec", "oob", "flag"):
            if fld in e and e.get("kind") is None:
                assert int(got[fld][k]) == e[fld], f"{name}: {fld} = {int(got[fld][k])}, expected {e[fld]} (flag {bool(got['flag'][k])}, used {int(got['used'][k])}, oob {bool(got['oob'][k])})"
        if e.get("kind") == "must" and not got["flag"][k]:
            must_unflagged.append(name)
    assert not must_unflagged, f"within ACT_BAND / 2 of a float rounding boundary by the host's libm and not flagged: {must_unflagged}"
    ncapped, capped = capped_counts(A, got, flag_cap_over)
    figures["capped_cases"], figures["capped_flagged"] = ncapped, capped
    return figures


def assert_flag_cap(*counts):
    """Over all launches: at most 1 in 10^5 of the near-miss and random cases is flagged (`flag everything` does not pass)."""
    n, flagged = sum(c[0] for c in counts), sum(c[1] for c in counts)
    assert n >= RANDOM_UES and flagged <= n // FLAG_CAP_PER, f"{flagged} of the {n} near-miss and random cases are flagged: more than 1 in {FLAG_CAP_PER}"
