"""The device code that decides who gets a grant, away from every trial: the NOMA grouping of one sector (prach::noma_resolve_sector and its restatement
inside prach::noma_glibc_slot) and the reset-candidate resolver (prach::classify_event, prach::resolve_reset_candidates<1 | 4>).  A deterministic generator
of named cases no Monte-Carlo trial produces, their references — the pinned oracle's own per-sector function (oracle/noma_oracle.c, through
oracle.binding.noma_group_sector) and the sequential definition of the reset-candidate walk in plain Python — and the glue around
tests/tools/gpu_resolve_harness.hip (case file, result file, one child process per launch).  Shared by tests/test_resolve_cases_cpu.py and
tests/test_gpu_resolve_synthetic.py.  No GPU here; the constants of the product's headers come from `gpu_resolve_harness --constants`."""
import ctypes
import math
import struct

import numpy as np

import harness as H

INT_MAX = 2**31 - 1
MAGIC = 0x52534C56
HARNESS = "gpu_resolve_harness.hip"
D1_LOW, D1_HIGH, D_MAX = 644245094, 644245095, 2147483646  # the largest d1 with d1 / RAND_MAX < 0.3, the smallest without, the largest rand()
FILLER = 0x2AAAAAAA  # what lies in a stream in front of and behind a case's draws (even: as a d2 it picks the weaker UE; as a d1, < 0.3 does not hold)

_libm = ctypes.CDLL("libm.so.6")
_libm.log.restype = ctypes.c_double
_libm.log.argtypes = [ctypes.c_double]


def clog(x):
    """The C library's log (what the reference and the host-built activation table call)."""
    return _libm.log(float(x))


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def pairs_with(g_lo, g_hi):
    return 10 * clog(g_hi) - 10 * clog(g_lo) > 15.


def threshold_neighbours(g_lo):
    """(a, b): neighbouring doubles, a the largest g_hi for which 10 * log(g_hi) - 10 * log(g_lo) > 15. is false, b its successor, for which it is true
    (bisection over the doubles' bit patterns)."""
    lo, hi = _bits(g_lo * math.exp(1.4)), _bits(g_lo * math.exp(1.6))
    assert not pairs_with(g_lo, _from_bits(lo)) and pairs_with(g_lo, _from_bits(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pairs_with(g_lo, _from_bits(mid)):
            hi = mid
        else:
            lo = mid
    return _from_bits(lo), _from_bits(hi)


# ---- NOMA cases -------------------------------------------------------------------------------------------------------------------------------------------

class Sector:
    """One sector's transmitters: singletons on the preambles `pre` (ascending) with gains `gain`, two transmitters on each preamble of `collided`;
    draws[grant][which]; lg: a log table that is NOT the log of the gains (one crafted case), else None."""

    def __init__(self, pre, gain, draws, collided=(), lg=None):
        self.pre, self.gain = np.asarray(pre, dtype=np.int64), np.asarray(gain, dtype=np.float64)
        self.draws, self.collided = np.asarray(draws, dtype=np.int32).reshape(-1, 2), tuple(collided)
        self.lg = None if lg is None else np.asarray(lg, dtype=np.float64)
        assert len(self.pre) == len(self.gain) and (np.diff(self.pre) > 0).all() and not set(self.pre.tolist()) & set(self.collided)


class NomaCase:
    """sectors: {sector number: Sector} (nonsector: {0: ...}); budget: draws the stream holds for the whole case (None: exactly what the reference consumes)."""

    def __init__(self, name, nP, nG, nonsector, sectors, budget=None, perm_seed=0):
        self.name, self.nP, self.nG, self.nonsector, self.sectors, self.budget = name, int(nP), int(nG), int(nonsector), dict(sectors), budget
        assert all(0 <= s < (1 if nonsector else 6) for s in self.sectors) and 1 <= self.nP <= 64 and 1 <= self.nG <= 64
        for sec in self.sectors.values():
            assert len(sec.draws) == self.nG and (len(sec.pre) == 0 or sec.pre[-1] < self.nP) and all(p < self.nP for p in sec.collided)
        rng = np.random.default_rng(1000 + perm_seed)
        self.uid = {s: rng.permutation(64)[:len(sec.pre)] for s, sec in self.sectors.items()}  # mode 1: the UE index behind every singleton, never its lane
        # mode 2: the UE records of the slot, in an order of their own
        rows = [(s, int(p), k) for s, sec in self.sectors.items() for k, p in enumerate(sec.pre)] + \
               [(s, int(p), -1) for s, sec in self.sectors.items() for p in sec.collided for _ in (0, 1)]
        self.rows = [rows[i] for i in rng.permutation(len(rows))]
        self.pos0 = int(rng.integers(0, 6))

    def __repr__(self):
        return self.name


class SectorRef:
    """What the reference says about one sector: granted (positions in preamble order), consumed [(grant, which), ...], logs, and from a plain Python
    walk over the same logs: pairs formed, leftovers granted, whether the device-table bands apply (ambiguous)."""


def python_walk(gain, lg, nG, jstart=1):
    """The pairing in plain Python (NOMA.c:251-307 read directly): sorted positions, pairs (i, j) in the order formed, the i looked at."""
    n = len(gain)
    order = sorted(range(n), key=lambda k: (gain[k], k))  # the stable bubble sort with strict <
    l10 = [10 * lg[k] for k in order]
    free, pairs, looked = [True] * n, [], []
    for i in range(n - 1):
        if not free[i]:
            continue
        looked.append(i)
        for j in range(jstart, n):
            if free[j] and j != i and l10[j] - l10[i] > 15.:
                free[i] = free[j] = False
                pairs.append((i, j))
                break
    return order, l10, pairs, looked, [k for k in range(n) if free[k]]


def sector_reference(ob, sec, nG, nonsector, band):
    r = SectorRef()
    n = len(sec.pre)
    r.count = n
    granted, r.consumed, r.logs = ob.noma_group_sector(np.arange(n), sec.gain, nG, nonsector, sec.draws, logs_in=sec.lg)
    assert len(set(granted)) == len(granted)
    r.granted = sorted(granted)
    r.pairs, r.leftovers_granted, r.ambiguous, r.order = 0, 0, False, list(range(n))
    if n > nG:
        order, l10, pairs, looked, left = python_walk(sec.gain, r.logs, nG)
        r.order, r.pairs, r.pair_list = order, len(pairs), pairs
        r.leftovers_granted = min(len(left), max(0, nG - len(pairs)))
        g = [sec.gain[k] for k in order]
        # the two bands as prach_noma_resolve.h defines them (sorted neighbours within ACT_GAIN_ORDER_BAND of the larger; a difference within 1e-9 of 15 seen
        # from an i that is looked at): a restatement, not an independent definition — the crafted twins inside and outside each band pin it by name
        r.ambiguous = any(g[k + 1] - g[k] <= band * g[k + 1] for k in range(n - 1)) or any(abs((l10[j] - l10[i]) - 15.0) < 1e-9 for i in looked for j in range(n))
    return r


def case_reference(ob, case, consts):
    """Per sector in order: the SectorRef, the draws it may take (`taken`, cut by the budget), its status and grants as the kernels must leave them; the
    case's stream and final position.  Sectors behind an exhausted one are not reached (status None)."""
    band = consts["ACT_GAIN_ORDER_BAND"]
    out, stream, used, status = {}, [], 0, consts["PRACH_OK"]
    total = sum(len(sector_reference(ob, sec, case.nG, case.nonsector, band).consumed) for sec in case.sectors.values())
    budget = total if case.budget is None else case.budget
    for s in sorted(case.sectors):
        sec = case.sectors[s]
        r = sector_reference(ob, sec, case.nG, case.nonsector, band)
        r.reached = status == consts["PRACH_OK"]
        r.budget = max(0, budget - used)
        need = len(r.consumed)
        r.status = consts["PRACH_OK"] if need <= r.budget else consts["PRACH_ERR_STREAM"]
        r.taken = r.consumed[:min(need, r.budget)]
        r.grants = r.granted if r.status == consts["PRACH_OK"] else []
        stream += [int(sec.draws[g, w]) for g, w in r.consumed]
        if r.reached:
            used += len(r.taken)
            status = r.status
        out[s] = r
    return out, stream, used, status


def _table(nG, d1, d2):
    return np.array([[d1, d2]] * nG, dtype=np.int32)


def _one(name, gain, nG, nonsector=0, draws=None, nP=None, pre=None, sector=0, budget=None, collided=(), lg=None, seed=0):
    n = len(gain)
    pre = np.arange(n) if pre is None else pre
    nP = max(int(pre[-1]) + 1 if n else 1, 1 + max(collided, default=0)) if nP is None else nP
    draws = _table(nG, D_MAX, 1) if draws is None else draws
    return NomaCase(name, nP, nG, nonsector, {0 if nonsector else sector: Sector(pre, gain, draws, collided, lg)}, budget, seed)


def _loguniform(rng, n, decades):
    return np.exp(rng.uniform(math.log(1e-6), math.log(1e-6) + decades * math.log(10), n))


RANDOM_DECADES = 3.0  # (10 ln of the whole range = 69: partners 15 apart are the rule; chosen for the coverage shares tests/test_resolve_cases_cpu.py asserts)
N_RANDOM = 700
G_LOS = (1e-7, 3.3e-5, 0.0123, 1.0, 57.25)


def noma_cases(consts):
    """Every crafted case, then the random sweep: N_RANDOM cases of six sectors (one when cell-wide), 3500 sectors in all — a sector is what one wavefront
    resolves, and the sectors are the 'few thousand' of the sweep.  Names are fixed (NOMA_CASE_NAMES); consts: `gpu_resolve_harness --constants`."""
    cases = []
    rng = np.random.default_rng(7)
    nG0 = 3
    for k, (label, count, nP) in enumerate((("1", 1, 54), ("2", 2, 54), ("ngrant", nG0, 54), ("ngrant_plus_1", nG0 + 1, 54), ("63", 63, 64), ("64", 64, 64))):
        pre = np.sort(rng.permutation(nP)[:count])
        cases.append(_one(f"count_{label}", _loguniform(rng, count, 3), nG0, draws=_table(nG0, D_MAX, 1), nP=nP, pre=pre, sector=k % 6, seed=k))
    # 64 singletons, 63 gains within 10 % of each other and one e^1.6 above them: sorted lane 0 pairs sorted lane 63, lanes 1 .. 62 look and find nobody
    g64 = np.concatenate([np.full(62, 1.0) * (1 + np.arange(62) * 1e-3), [1.1, 1.1 * math.exp(1.6)]])
    cases.append(_one("count_64_pairs_lane_63", g64[rng.permutation(64)], 40, draws=_table(40, D_MAX, 1), nP=64, sector=1, seed=11))
    cases.append(_one("tie_all_equal", np.full(5, 0.25), 2, sector=2, seed=12))
    cases.append(_one("tie_decides_who_pairs", [100.0, 1.0, 100.0], 1, sector=3, seed=13))
    cases.append(_one("chain_nearest_admissible", np.exp(0.8 * np.arange(8))[[3, 0, 7, 1, 6, 2, 5, 4]], 4, draws=np.array([[D_MAX, 0], [D1_LOW, 1], [D1_LOW, 2], [0, 3]]),
                      sector=4, seed=14))
    cases.append(_one("nobody_pairs", [1.9, 1.0, 1.3, 1.7, 1.1, 1.5], 3, sector=5, seed=15))
    # the only way sorted lane 0 can be an admissible partner: a table whose logs do not follow its gains (a device-built table is not required to be monotone)
    cases.append(_one("lane0_only_admissible_partner", [1.0, 2.0, 3.0, 4.0], 2, lg=[3.0, 0.1, 0.2, 0.3], sector=0, seed=16))
    cases.append(_one("more_pairs_than_grants", np.exp(1.6 * np.arange(6)), 1, draws=_table(1, D1_LOW, 1), sector=1, seed=17))
    cases.append(_one("more_pairs_than_grants_nonsector", np.exp(1.6 * np.arange(7)), 1, nonsector=1, draws=_table(1, D1_LOW, 1), seed=18))
    cases.append(_one("collided_preambles_stay_out", [1.0, 40.0, 2.0, 90.0], 2, pre=np.array([1, 4, 9, 30]), nP=54, collided=(0, 5, 53), sector=2, seed=19))
    for q, g_lo in enumerate(G_LOS):
        a, b = threshold_neighbours(g_lo)
        for label, g_hi in (("below", a), ("above", b), ("minus_1e-10", g_lo * math.exp(1.5 - 1e-11)), ("plus_1e-10", g_lo * math.exp(1.5 + 1e-11)),
                            ("minus_1e-8", g_lo * math.exp(1.5 - 1e-9)), ("plus_1e-8", g_lo * math.exp(1.5 + 1e-9))):
            cases.append(_one(f"threshold_{q}_{label}", [g_hi, g_lo], 1, sector=q % 6, nonsector=q == 3, seed=20 + q))
    band = consts["ACT_GAIN_ORDER_BAND"]  # (the compiled value: the gaps below are 0.75 and 1.5 times it)
    for q, ga in enumerate((1e-5, 0.7, 33.0)):
        for label, rel in (("inside", 0.75 * band), ("outside", 1.5 * band)):
            cases.append(_one(f"order_band_{q}_{label}", [3 * ga, ga * (1 + rel), ga], 2, sector=q, seed=30 + q))
    for q, (d1, d2) in enumerate(((0, 0), (0, 1), (D1_LOW, 2), (D1_LOW, D_MAX - 1), (D1_HIGH, 0), (D1_HIGH, 1), (D_MAX, 0), (D_MAX, 1))):
        for nonsector in (0, 1):
            cases.append(_one(f"draws_d1_{d1}_d2_{'odd' if d2 % 2 else 'even'}{'_nonsector' if nonsector else ''}", [1.0, 5.0, 0.5, 4.0, 9.0], 2,
                              draws=_table(2, d1, d2), nonsector=nonsector, sector=q % 6, seed=40 + q))
    # budgets: two pairs, each taking two draws
    gb, db = np.exp(1.6 * np.arange(4))[[2, 0, 3, 1]], np.array([[D1_LOW, 1], [0, 2]])
    for label, budget in (("first_draw_of_grant_0", 0), ("second_draw_of_grant_0", 1), ("first_draw_of_grant_1", 2), ("second_draw_of_grant_1", 3), ("exactly_enough", 4)):
        cases.append(_one(f"budget_{label}", gb, 2, draws=db, budget=budget, sector=3, seed=50))
    # six sectors that all consume draws: the stream position carries from sector to sector; and a budget that ends in the fourth
    def six(name, budget, seed, d1s=(0, D1_LOW, D1_HIGH, D_MAX)):
        r = np.random.default_rng(seed)
        secs = {}
        for s in range(6):
            n = 6 + 2 * s
            d = np.stack([r.choice(d1s, 3), r.integers(0, D_MAX, 3)], axis=1)
            secs[s] = Sector(np.sort(r.permutation(54)[:n]), np.exp(1.7 * r.permutation(n)), d, collided=())
        return NomaCase(name, 54, 3, 0, secs, budget, seed)
    cases.append(six("six_sectors_position_carries", None, 60))
    cases.append(six("six_sectors_budget_ends_in_a_later_sector", 15, 60, (D1_LOW,)))  # (every sector forms three pairs or more: six draws each, three of the third's)
    cases.append(six("six_sectors_budget_ends_at_a_sector_start", 6, 61, (D_MAX,)))    # (three draws each: none left for the third)
    # the random sweep
    rng = np.random.default_rng(77)
    for k in range(N_RANDOM):
        nonsector = int(k % 5 == 4)
        nG = int(rng.integers(1, 41))
        secs = {}
        for s in range(1 if nonsector else 6):
            count = int(rng.integers(1, 65))
            nP = 64
            pre = np.sort(rng.permutation(nP)[:count])
            free = np.setdiff1d(np.arange(nP), pre)
            coll = tuple(int(v) for v in rng.permutation(free)[:int(rng.integers(0, 3))])
            d = np.stack([rng.choice([0, D1_LOW, D1_HIGH, D_MAX, int(rng.integers(0, D_MAX))], nG), rng.integers(0, D_MAX + 1, nG)], axis=1)
            secs[s] = Sector(pre, _loguniform(rng, count, RANDOM_DECADES), d, coll)
        cases.append(NomaCase(f"random_{k:03d}", 64, nG, nonsector, secs, None if k % 7 else int(rng.integers(0, 12)), 100 + k))
    return cases


def _crafted_names():
    n = [f"count_{c}" for c in ("1", "2", "ngrant", "ngrant_plus_1", "63", "64")]
    n += ["count_64_pairs_lane_63", "tie_all_equal", "tie_decides_who_pairs", "chain_nearest_admissible", "nobody_pairs", "lane0_only_admissible_partner",
          "more_pairs_than_grants", "more_pairs_than_grants_nonsector", "collided_preambles_stay_out"]
    n += [f"threshold_{q}_{label}" for q in range(len(G_LOS)) for label in ("below", "above", "minus_1e-10", "plus_1e-10", "minus_1e-8", "plus_1e-8")]
    n += [f"order_band_{q}_{label}" for q in range(3) for label in ("inside", "outside")]
    n += [f"draws_d1_{d1}_d2_{par}{ns}" for d1, par in ((0, "even"), (0, "odd"), (D1_LOW, "even"), (D1_LOW, "odd"), (D1_HIGH, "even"), (D1_HIGH, "odd"), (D_MAX, "even"),
                                                         (D_MAX, "odd")) for ns in ("", "_nonsector")]
    n += [f"budget_{b}" for b in ("first_draw_of_grant_0", "second_draw_of_grant_0", "first_draw_of_grant_1", "second_draw_of_grant_1", "exactly_enough")]
    n += ["six_sectors_position_carries", "six_sectors_budget_ends_in_a_later_sector", "six_sectors_budget_ends_at_a_sector_start"]
    return tuple(n)


NOMA_CRAFTED_NAMES = _crafted_names()
NOMA_CASE_NAMES = NOMA_CRAFTED_NAMES + tuple(f"random_{k:03d}" for k in range(N_RANDOM))
# the cases whose sectors a device-built table must report (devact = 1), and their twins just outside, which it must not
AMBIGUOUS_NAMES = ("tie_all_equal", "tie_decides_who_pairs") + tuple(f"threshold_{q}_{label}" for q in range(len(G_LOS)) for label in
                                                                      ("below", "above", "minus_1e-10", "plus_1e-10")) + tuple(f"order_band_{q}_inside" for q in range(3))
CLEAR_TWIN_NAMES = tuple(f"threshold_{q}_{label}" for q in range(len(G_LOS)) for label in ("minus_1e-8", "plus_1e-8")) + tuple(f"order_band_{q}_outside" for q in range(3))


# ---- reset-candidate cases --------------------------------------------------------------------------------------------------------------------------------

class ResetCase:
    def __init__(self, name, nP, NB, fcall, events, only_count=False):
        self.name, self.nP, self.NB, self.only_count = name, int(nP), int(NB), only_count
        self.fcall, self.events = np.ascontiguousarray(fcall, dtype=np.int32), np.ascontiguousarray(events, dtype=np.int32).reshape(-1, 2)
        assert len(self.fcall) == nP and nP <= (64 if NB == 1 else 256)
        assert len(set(self.events[:, 0].tolist())) == len(self.events) and (self.events[:, 0] >= 0).all() and (self.events[:, 0] < 2**20).all()

    def __repr__(self):
        return self.name


def ev_info(typ, p, q=0, ispre=0):
    """type[2:0] ispre[3] bucket p[11:4] old bucket q[19:12] (prach_resolve.h)"""
    return typ | (ispre << 3) | (p << 4) | (q << 12)


def reset_reference(case, consts):
    """The sequential definition: classify every event against the initial table; walk the survivors in ascending index; a survivor is void if
    fcall[q] < idx, otherwise it sets fcall[p] = idx when idx < fcall[p]."""
    fc = [int(v) for v in case.fcall]
    nP, nev = case.nP, len(case.events)
    void, nlv, fie, nrj, surv = [0] * nev, [0] * nP, [0] * nP, 0, []
    for k, (idx, info) in enumerate(case.events.tolist()):
        typ, p, q = info & 7, (info >> 4) & 0xff, (info >> 12) & 0xff
        if typ == consts["UEV_RESETCAND"]:
            if fc[q] < idx:
                void[k] = 1
            else:
                surv.append((idx, p, q, k))
        elif typ == consts["UEV_RJOIN"]:
            nrj += 1
        elif typ == consts["EV_LEAVER"]:
            nlv[p] += idx < fc[p]
        elif typ == consts["UEV_CALLER"]:
            if idx == fc[p]:
                fie[p] = 1
    resolved = len(surv) <= consts["RCCAP"]
    rejoined = 0
    if resolved:
        for idx, p, q, k in sorted(surv):
            if fc[q] < idx:
                void[k] = 1
            else:
                rejoined += 1
                if idx < fc[p]:
                    fc[p] = idx
    return dict(nrc=len(surv), nrj=nrj, resolved=int(resolved), fcall=fc, nlv=nlv, fie=fie, void=void, bumped_by_rejoin=len(surv) - rejoined if resolved else None,
                killed_by_definite=sum(void) - (len(surv) - rejoined) if resolved else None)


def _reset_build(rng, consts, name, nP, NB, nsurv, nkill=0, ncall=0, nleave=0, nrj=0, buckets=None, chain=None, shuffle=True, only_count=False, free_share=0.5,
                 lead=0):
    """buckets: the buckets candidates use (default: all); chain: None, or the number of leading survivors linked p_k = q_{k+1} over buckets that nobody
    called (their fate then alternates along the chain from the first one's); lead: 1 puts one survivor of its own bucket in front of the chain, which
    moves every chain member one place along the blocks of 64."""
    RC, CALL, LEAVE, RJ = consts["UEV_RESETCAND"], consts["UEV_CALLER"], consts["EV_LEAVER"], consts["UEV_RJOIN"]
    B = np.arange(nP) if buckets is None else np.asarray(buckets)
    fcall = np.full(nP, INT_MAX, dtype=np.int64)
    called = B[rng.random(len(B)) >= free_share] if nP > 1 else np.array([], dtype=np.int64)
    if len(called) == len(B):
        called = called[:-1]  # (one bucket nobody called: a survivor of any index has an old bucket to come from)
    total = nsurv + nkill + ncall + nleave + nrj
    pool = rng.permutation(np.arange(1000, 2**20 - 1000, 3))[:total + len(called)].tolist()  # (distinct, and idx - 1, idx + 1 are nobody's)
    for b in called:
        fcall[b] = pool.pop()
    if len(called) and nkill:
        fcall[called[0]] = 999  # somebody every candidate can be bumped by
    events = []
    cidx = sorted(pool.pop() for _ in range(nsurv))
    freeb = B[fcall[B] == INT_MAX]
    assert len(freeb) or nsurv == 0
    for k, idx in enumerate(cidx):
        if lead and k == 0:
            q = p = int(freeb[-1])
        elif chain and k < chain:
            q, p = int(freeb[(k - lead) % len(freeb)]), int(freeb[(k - lead + 1) % len(freeb)])
        else:
            ok = B[fcall[B] >= idx]
            q, p = int(rng.choice(ok)), int(rng.choice(B))
            if rng.integers(0, 8) == 0:
                p = q
        events.append((idx, ev_info(RC, p, q, int(rng.integers(0, 2)))))
    for _ in range(nkill):
        idx = pool.pop()
        low = B[fcall[B] < idx]
        if not len(low):
            continue  # (every bucket in use is free: nobody can be bumped at classification)
        events.append((idx, ev_info(RC, int(rng.choice(B)), int(rng.choice(low)))))
    for k in range(ncall):  # every other one IS its bucket's first caller (its index is the table's), the others call behind it
        p = int(called[k % len(called)]) if len(called) else int(rng.choice(B))
        idx = pool.pop()
        if k < len(called) and k % 2 == 0:
            idx = int(fcall[p])
        elif len(called):
            idx = max(idx, int(fcall[p]) + 2 + 3 * k)
        events.append((idx, ev_info(CALL, p, 0, int(rng.integers(0, 2)))))
    for k in range(nleave):  # just below and just above the bucket's first caller
        pool.pop()
        if len(called):
            p = int(called[k % len(called)])
            idx = int(fcall[p]) + (-1 if (k // len(called)) % 2 == 0 else 1)
        else:
            p, idx = int(rng.choice(B)), 5 + k
        events.append((idx, ev_info(LEAVE, p)))
    for _ in range(nrj):
        events.append((pool.pop(), ev_info(RJ, int(rng.choice(B)))))
    seen, uniq = set(), []
    for e in events:  # (a leaver next to a caller that moved, or two around one caller: the first of an index stays)
        if e[0] not in seen and 0 <= e[0] < 2**20:
            seen.add(e[0])
            uniq.append(e)
    ev = np.array(uniq, dtype=np.int64).reshape(-1, 2)
    if shuffle and len(ev):
        ev = ev[rng.permutation(len(ev))]
    return ResetCase(name, nP, NB, fcall, ev, only_count)


SURVIVOR_COUNTS = (0, 1, 63, 64, 65, 128, 255, 256)
NB1_NP, NB4_NP = (1, 2, 54, 63, 64), (65, 128, 129, 192, 193, 254)
N_RESET_RANDOM = 150


def _edges(nP):
    return sorted({b for b in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, nP - 2, nP - 1) if 0 <= b < nP})


def reset_cases(consts):
    cases = []
    rng = np.random.default_rng(5)
    for n in SURVIVOR_COUNTS:
        for NB, nP in ((1, 64), (4, 254)):
            cases.append(_reset_build(rng, consts, f"survivors_{n}_nb{NB}", nP, NB, n, nkill=20, ncall=30, nleave=40, nrj=5))
    cases.append(_reset_build(rng, consts, "survivors_257_only_counted", 254, 4, 257, nkill=10, ncall=10, nleave=10, nrj=3, only_count=True))
    cases.append(_reset_build(rng, consts, "survivors_exactly_rccap_few_buckets", 8, 1, consts["RCCAP"], nkill=30, ncall=8, nleave=16, nrj=2))
    # chains p_k = q_{k+1} across the 64-candidate block edges: the first candidate of every block re-joins and every second one is bumped; with one
    # survivor of a bucket of its own in front, the first candidate of the second block is a bumped one and every later fate sits one place further.  All buckets free, so nothing but the chain decides
    for NB, nP in ((1, 64), (4, 254)):
        for label, lead in (("first_rejoins", 0), ("first_bumped", 1)):
            cases.append(_reset_build(np.random.default_rng(9), consts, f"chain_{label}_nb{NB}", nP, NB, 200 + lead, chain=200 + lead, free_share=1.1, lead=lead))
    cases.append(_reset_build(rng, consts, "chain_then_crowd_nb4", 254, 4, 256, nkill=40, ncall=20, nleave=20, chain=100))
    cases.append(_reset_build(rng, consts, "few_buckets_p_equals_q_nb1", 2, 1, 70, nkill=10, ncall=2, nleave=8, nrj=1, free_share=0.5))
    cases.append(_reset_build(rng, consts, "bumped_by_definite_caller_and_by_rejoin", 16, 1, 120, nkill=60, ncall=10, nleave=20))
    cases.append(_reset_build(rng, consts, "leavers_and_callers_around_the_first_caller", 54, 1, 10, nkill=5, ncall=54, nleave=108, nrj=7, free_share=0.15))
    cases.append(_reset_build(rng, consts, "events_in_ascending_order", 54, 1, 90, nkill=20, ncall=20, nleave=20, nrj=4, shuffle=False))
    for nP in NB1_NP:
        cases.append(_reset_build(rng, consts, f"nb1_np{nP}", nP, 1, 100, nkill=15 if nP > 1 else 0, ncall=2 * nP, nleave=2 * nP, nrj=3))
    for nP in NB4_NP:
        cases.append(_reset_build(rng, consts, f"nb4_np{nP}_register_edges", nP, 4, 200, nkill=30, ncall=40, nleave=40, nrj=3, buckets=_edges(nP)))
        cases.append(_reset_build(rng, consts, f"nb4_np{nP}", nP, 4, 130, nkill=30, ncall=nP, nleave=nP, nrj=3))
    rng = np.random.default_rng(55)
    for k in range(N_RESET_RANDOM):
        NB = 1 if k % 2 == 0 else 4
        nP = int(rng.integers(1, 65)) if NB == 1 else int(rng.integers(1, 255))
        nsurv = int(rng.choice([0, 1, 5, 63, 64, 65, 100, 130, 200, 256])) if k % 3 else int(rng.integers(0, 257))
        few = _edges(nP) if k % 5 == 0 else (rng.permutation(nP)[:max(1, nP // 8)] if k % 5 == 1 else None)
        cases.append(_reset_build(rng, consts, f"random_{k:03d}_nb{NB}", nP, NB, nsurv, nkill=int(rng.integers(0, 60)) if nP > 1 else 0, ncall=int(rng.integers(0, 80)),
                                  nleave=int(rng.integers(0, 80)), nrj=int(rng.integers(0, 6)), buckets=few, chain=int(rng.integers(0, nsurv + 1)) if k % 4 == 0 else None,
                                  free_share=float(rng.choice([0.2, 0.5, 0.9]))))
    return cases


def _reset_names():
    n = [f"survivors_{c}_nb{NB}" for c in SURVIVOR_COUNTS for NB in (1, 4)] + ["survivors_257_only_counted", "survivors_exactly_rccap_few_buckets"]
    n += [f"chain_{label}_nb{NB}" for NB in (1, 4) for label in ("first_rejoins", "first_bumped")]
    n += ["chain_then_crowd_nb4", "few_buckets_p_equals_q_nb1", "bumped_by_definite_caller_and_by_rejoin", "leavers_and_callers_around_the_first_caller",
          "events_in_ascending_order"]
    n += [f"nb1_np{nP}" for nP in NB1_NP]
    for nP in NB4_NP:
        n += [f"nb4_np{nP}_register_edges", f"nb4_np{nP}"]
    return tuple(n) + tuple(f"random_{k:03d}_nb{1 if k % 2 == 0 else 4}" for k in range(N_RESET_RANDOM))


RESET_CASE_NAMES = _reset_names()


# ---- the harness ------------------------------------------------------------------------------------------------------------------------------------------

def build_harness(out_dir):
    """Compiles tests/tools/gpu_resolve_harness.hip (host program + the three wrapper kernels for gfx950, the product's -ffp-contract=off) into out_dir."""
    return H.build(HARNESS, out_dir, ["-ffp-contract=off"])


def harness_constants(exe):
    return H.constants(exe, lambda v: float.fromhex(v) if "x" in v else int(v))  # (ACT_GAIN_ORDER_BAND is a hexadecimal float)


def _header(mode, ncases):
    h = np.zeros(16, dtype="<i4")
    h[:3] = [MAGIC, mode, ncases]
    return h


def write_mode1(path, units, consts):
    """units: [(case, sector number, budget), ...], one wavefront each."""
    W = consts["M1_WORDS"]
    rec = np.zeros((len(units), W), dtype="<i4")
    for k, (case, s, budget) in enumerate(units):
        sec, uid = case.sectors[s], case.uid[s]
        r = rec[k]
        r[0:3] = [case.nG, case.nonsector, budget]
        r[4:68] = -1
        r[4 + sec.pre] = uid
        r[68:68 + 2 * case.nG] = sec.draws.reshape(-1)
        gain, lgain = np.full(64, -1.0), np.full(64, 1e300)
        gain[uid] = sec.gain
        lgain[uid] = [clog(g) for g in sec.gain] if sec.lg is None else sec.lg
        r[196:324] = gain.astype("<f8").view("<i4")
        r[324:452] = lgain.astype("<f8").view("<i4")
    with open(path, "wb") as f:
        f.write(_header(1, len(units)).tobytes())
        f.write(rec.tobytes())


def read_mode1(path, units, consts, devact):
    r = np.fromfile(path, dtype="<i4")
    assert r[:4].tolist() == [MAGIC, 1, devact, len(units)] and r.size == 4 + len(units) * consts["M1_RES"]
    r = r[4:].reshape(len(units), consts["M1_RES"])
    out = []
    for k, (case, s, _) in enumerate(units):
        uid = case.uid[s]
        assert not np.delete(r[k, :64], uid).any(), f"{case.name} sector {s}: a grant for a UE index that is not in the sector"
        nt = int(r[k, 64])
        out.append(dict(granted=[i for i, u in enumerate(uid) if r[k, u]], taken=[(int(v) // 2, int(v) % 2) for v in r[k, 65:65 + nt]], status=int(r[k, 193]),
                        ambiguous=int(r[k, 194])))
    return out


def write_mode2(path, cases, streams):
    """streams[k]: the draws the reference consumes in case k, in order.  The stream of a case: pos0 filler values, the draws, filler; stream_len = pos0 +
    the budget."""
    tab = np.zeros((len(cases), 8), dtype="<i4")
    parts = []
    for k, (case, st) in enumerate(zip(cases, streams)):
        budget = len(st) if case.budget is None else case.budget
        stream = [FILLER] * case.pos0 + list(st) + [FILLER] * (4 + max(0, budget - len(st)))
        tab[k, :7] = [len(case.rows), case.nP, case.nG, case.nonsector, case.pos0, budget, len(stream)]
        ue = np.zeros((len(case.rows), 8), dtype="<i4")
        g = np.zeros((len(case.rows), 2), dtype="<f8")
        for i, (s, p, pos) in enumerate(case.rows):
            sec = case.sectors[s]
            ue[i, 0], ue[i, 1] = s, p
            if pos >= 0:
                g[i] = [sec.gain[pos], clog(sec.gain[pos]) if sec.lg is None else sec.lg[pos]]
            else:
                g[i] = [1e6, 50.0]  # a collided transmitter: the strongest of all, were it looked at
        ue[:, 4:8] = g.view("<i4")
        parts += [ue.reshape(-1), np.array(stream, dtype="<i4")]
    with open(path, "wb") as f:
        f.write(_header(2, len(cases)).tobytes())
        f.write(tab.tobytes())
        for p in parts:
            f.write(np.ascontiguousarray(p, dtype="<i4").tobytes())


def read_mode2(path, cases, devact):
    r = np.fromfile(path, dtype="<i4")
    assert r[:4].tolist() == [MAGIC, 2, devact, len(cases)]
    o, out = 4, []
    for case in cases:
        n = len(case.rows)
        msg2 = r[o:o + n]
        granted = {s: sorted(pos for (s2, _, pos), m in zip(case.rows, msg2) if s2 == s and pos >= 0 and m) for s in case.sectors}
        assert set(msg2.tolist()) <= {0, 1} and not any(m for (_, _, pos), m in zip(case.rows, msg2) if pos < 0), f"{case.name}: msg2 of a collided transmitter"
        out.append(dict(granted=granted, pos=int(r[o + n]), status=int(r[o + n + 1])))
        o += n + 4
    assert o == r.size
    return out


def write_mode3(path, cases):
    tab = np.zeros((len(cases), 8), dtype="<i4")
    with open(path, "wb") as f:
        for k, c in enumerate(cases):
            tab[k, :3] = [c.nP, c.NB, len(c.events)]
        f.write(_header(3, len(cases)).tobytes())
        f.write(tab.tobytes())
        for c in cases:
            f.write(c.fcall.astype("<i4").tobytes())
            f.write(c.events.astype("<i4").tobytes())


def read_mode3(path, cases):
    r = np.fromfile(path, dtype="<i4")
    assert r[:4].tolist() == [MAGIC, 3, 0, len(cases)]
    o, out = 4, []
    for c in cases:
        nP, nev = c.nP, len(c.events)
        out.append(dict(nrc=int(r[o]), nrj=int(r[o + 1]), resolved=int(r[o + 2]), fcall=r[o + 4:o + 4 + nP].tolist(), nlv=r[o + 4 + nP:o + 4 + 2 * nP].tolist(),
                        fie=r[o + 4 + 2 * nP:o + 4 + 3 * nP].tolist(), void=r[o + 4 + 3 * nP:o + 4 + 3 * nP + nev].tolist()))
        o += 4 + 3 * nP + nev
    assert o == r.size
    return out


def run_harness(exe, case_path, result_path, devact, timeout=120):
    """One launch in a fresh child process (harness.run)."""
    H.run(exe, [case_path, result_path, devact], timeout)
