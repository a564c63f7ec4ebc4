"""The exact CPU reference of NOMA.c's channel trace (include/prach.h, prach_noma_trace), from the ORACLE alone: it never calls the library.  Two independent
views of a trial (tests/tools/NOMA_TRACE.md):

  * the sector hook (oracle.binding.noma_run_trial_traced) gives, for every (slot, sector) with a singleton, singles (the length of idx), granted, and the decode
    draws: pairs is the number of draws with which == 0, pair_one those of them with a value <= 644245094 (the integer form of < 0.3);
  * tx and used come from two STOPPED runs: the UEs of the run cut at max_steps = t that satisfy the gather's condition (NOMA.c:207), counted with their sector
    and preamble, plus the new arrivals of subframe t — the indices from that run's activeCheck up to the activeCheck of the run cut at t + 1, with the sector
    and preamble that second run holds (the trace cases keep maxMsg1ReTx >= 2: a first transmission cannot redraw its preamble).  max_steps = 0 means "no cut":
    slot 0 takes everything from the run cut at 1.

The self-check ties the two: the bins with exactly one transmitter are the hook's count.  A stopped run costs 5 to 300 ms, so tx and used are computed at the
slots a caller names; the other four at every slot.  The re-binning and the scalars are restated in numpy.  No GPU, no package import."""
import numpy as np

SERIES = ("tx", "used", "singles", "granted", "pairs", "pair_one")
TX, USED, SINGLES, GRANTED, PAIRS, PAIR_ONE = range(6)
SCALARS = ("trials", "slots", "tx", "used", "singles", "granted", "pairs", "pair_one", "overflow_tx", "tx_max")
ONE_OF_TWO = 644245094
MAX_TIME = 10000
# columns of the 16-word record (the oracle's noma_ue and the product's log)
W_ACTIVE, W_TXTIME, W_NOWBACKOFF, W_PREAMBLE, W_SECTOR, W_MSG2, W_RA, W_FAIL = 2, 3, 6, 7, 8, 12, 14, 15


# The trial cases, in the library's config terms (maxMsg2TxCount is NOMA.c's maxMsg1ReTx; flags = 2: the cell-wide grouping); all Philox.  `every`: tx and used
# are checked at every `every`-th slot (1: all of them, on the smallest case)
CASES = {
    "all_states": dict(nUE=2000, seed=6, nGrantUL=1, maxMsg2TxCount=3, max_steps=4325),          # the census' all-states trial
    "all_states_partial": dict(nUE=2000, seed=6, nGrantUL=1, maxMsg2TxCount=3, max_steps=4323),  # ... with a partial last slot
    "cellwide": dict(nUE=1500, seed=9, nPreamble=3, flags=2, nGrantUL=1, maxMsg2TxCount=2, max_steps=5000),  # collided bins in most busy slots; sectors 1-5 zero
    "last_preamble": dict(nUE=6000, seed=3, nPreamble=64, accessTime=10, nGrantUL=3, backoff=40, max_steps=3000),  # lane == last preamble; slot != 5 ms
    "cluster": dict(nUE=20000, seed=7, nGrantUL=2, maxMsg2TxCount=3, max_steps=2600),            # only workgroup 0 writes, and it writes cluster totals
    "rar6": dict(nUE=3000, seed=5, maxRarWindow=6, max_steps=4000),                              # a failed transmitter is never rescheduled
    "full_run": dict(nUE=300, seed=1),                                                           # all 2000 slots (at 300 UEs no seed of 0..23 serves every UE: no exit)
    "early_exit": dict(nUE=100, seed=5),                                                         # every UE served at subframe 511: rows behind time_exit zero
}
EVERY = {"all_states": 16, "all_states_partial": 16, "cellwide": 8, "last_preamble": 10, "cluster": 40, "rar6": 25, "full_run": 100, "early_exit": 1}


def case_oracle_cfg(ob, case):
    k = dict(CASES[case])
    k.pop("seed")
    if "maxMsg2TxCount" in k:
        k["maxMsg1ReTx"] = k.pop("maxMsg2TxCount")
    k["nonsector"] = 1 if k.pop("flags", 0) & 2 else 0
    return ob.make_noma_cfg(k.pop("nUE"), **k)


_trials = {}


def case_trial(ob, case):
    """(oracle cfg, res, rows, mask, UEs) of a case, computed once per process and left unchanged."""
    if case not in _trials:
        oc, seed = case_oracle_cfg(ob, case), CASES[case]["seed"]
        res0, _ = ob.noma_run_trial(oc, ob.Rng(ob.RNG_PHILOX, seed), want_ues=False)
        res, rows, mask = trial_rows(ob, oc, seed, spread(nslots(res0.steps, oc.accessTime), EVERY[case]))
        _, ues = run(ob, oc, seed)
        rows.setflags(write=False)
        _trials[case] = (oc, res, rows, mask, ues)
    return _trials[case]


def as_array(ues):
    """The oracle's NomaUE array (16 int32 + a double) or a product log (16 int32) as int32 [nUE, 16]."""
    n = len(ues)
    return np.frombuffer(ues, dtype=np.uint8).reshape(n, -1)[:, :64].copy().view(np.int32).reshape(n, 16)


def oracle_cfg(ob, c, max_steps=None):
    """The oracle's config of a library config (maxMsg2TxCount is NOMA.c's maxMsg1ReTx; flag 2 is the cell-wide grouping)."""
    return ob.make_noma_cfg(c.nUE, nPreamble=c.nPreamble, backoff=c.backoff, nGrantUL=c.nGrantUL, maxRarWindow=c.maxRarWindow, maxMsg1ReTx=c.maxMsg2TxCount,
                            accessTime=c.accessTime, max_steps=c.max_steps if max_steps is None else max_steps, cellRadius=c.cellRadius, nonsector=1 if c.flags & 2 else 0)


def stop_of(oc):
    return oc.max_steps if 0 < oc.max_steps < MAX_TIME else MAX_TIME


def run(ob, oc, seed):
    res, ues = ob.noma_run_trial(oc, ob.Rng(ob.RNG_PHILOX, seed))
    return res, as_array(ues)


def nslots(steps, access_time):
    """The slots whose subframe lies in [0, E), E = min(steps, maxTime)."""
    E = min(int(steps), MAX_TIME)
    return (E + access_time - 1) // access_time


def resolved(ob, oc, seed):
    """View 1.  (res, rows): rows int64 [slots, 6 sectors, 6 series] with singles, granted, pairs and pair_one of every slot; tx and used are left 0."""
    res, secs = ob.noma_run_trial_traced(oc, ob.Rng(ob.RNG_PHILOX, seed), cap_sectors=6 * (MAX_TIME // oc.accessTime + 1))
    rows = np.zeros((nslots(res.steps, oc.accessTime), 6, 6), dtype=np.int64)
    for r in secs:
        first = [v for (_, which, v) in r["draws"] if which == 0]
        rows[r["slot"], r["sector"], SINGLES:] = (len(r["idx"]), len(r["granted"]), len(first), sum(v <= ONE_OF_TWO for v in first))
    return res, rows


def gathered(ob, oc, seed, slot):
    """View 2.  The (sector, preamble) bin counts of one slot as int64 [6, nPreamble], or None if the trial never runs that slot (behind max_steps or an early
    exit)."""
    t = slot * oc.accessTime
    if t >= stop_of(oc):
        return None
    cut = lambda steps: run(ob, type(oc)(oc.nUE, oc.nPreamble, oc.backoff, oc.nGrantUL, oc.maxRarWindow, oc.maxMsg1ReTx, oc.accessTime, steps, oc.nonsector, oc.cellRadius), seed)
    cnt = np.zeros((6, oc.nPreamble), dtype=np.int64)
    ac = 0
    if t > 0:
        ra, a = cut(t)
        if ra.nSuccessUE == oc.nUE:  # NOMA.c:707-710 broke at or before subframe t - 1
            return None
        ac = int(ra.activeCheck)
        a = a[:ac].astype(np.int64)
        on = (a[:, W_RA] == 0) & (a[:, W_TXTIME] == t + 1) & (a[:, W_MSG2] == 0) & (a[:, W_NOWBACKOFF] <= 0) & ((a[:, W_FAIL] & 0xffff) == 0)
        np.add.at(cnt, (0 if oc.nonsector else a[on, W_SECTOR], a[on, W_PREAMBLE]), 1)
    rb, b = cut(t + 1)
    b = b[ac:int(rb.activeCheck)].astype(np.int64)  # activated at subframe t: every one of them transmits (txTime = t + 1, no backoff)
    np.add.at(cnt, (0 if oc.nonsector else b[:, W_SECTOR], b[:, W_PREAMBLE]), 1)
    return cnt


def spread(n, every):
    """A spread subset of the slots 0 .. n - 1: every `every`-th, the first two and the last two."""
    return sorted(set(range(0, n, every)) | {s for s in (0, 1, n - 2, n - 1) if 0 <= s < n})


def trial_rows(ob, oc, seed, slots):
    """(res, rows, mask): both views of one trial.  rows [slots, 6, 6] with tx and used filled in at the slots of `slots` (mask[s] True), and the self-check
    made there: the bins with exactly one transmitter are the hook's count, sector by sector."""
    res, rows = resolved(ob, oc, seed)
    mask = np.zeros(len(rows), dtype=bool)
    for s in slots:
        if s >= len(rows):
            continue
        cnt = gathered(ob, oc, seed, s)
        assert cnt is not None, (s, len(rows))
        rows[s, :, TX] = cnt.sum(axis=1)
        rows[s, :, USED] = (cnt >= 1).sum(axis=1)
        assert ((cnt == 1).sum(axis=1) == rows[s, :, SINGLES]).all(), ("self-check", s, (cnt == 1).sum(axis=1).tolist(), rows[s, :, SINGLES].tolist())
        mask[s] = True
    return res, rows, mask


def grants_of_ues(a):
    """sum_i (msg2_i + msg3Faile_i): every grant sets msg2, and only a failed Msg3 clears it again."""
    a = a.astype(np.int64)
    return int(a[:, W_MSG2].sum() + (a[:, W_FAIL] >> 16).sum())


def check_identities(rows, mask, nGrantUL, nPreamble):
    """The per-row identities of the record (tx and used where they are known)."""
    r = rows
    assert (r[..., PAIR_ONE] <= r[..., PAIRS]).all() and (r[..., PAIRS] <= nGrantUL).all() and (r[..., GRANTED] <= r[..., SINGLES]).all()
    m = r[mask]
    assert (m[..., SINGLES] <= m[..., USED]).all() and (m[..., USED] <= nPreamble).all() and (m[..., TX] >= 2 * m[..., USED] - m[..., SINGLES]).all()
    # a pair takes ONE grant of the budget and sets msg2 of two UEs, or of one: what the pairs leave of the budget goes to single UEs
    n_noma = 2 * r[..., PAIRS] - r[..., PAIR_ONE]
    assert (n_noma <= r[..., GRANTED]).all() and (r[..., GRANTED] - n_noma <= nGrantUL - r[..., PAIRS]).all()


def rebin(rows_list, access_times, bins, bin_ms, groups=None, ngroups=None):
    """The definition, in numpy: (series int64 [6, ngroups, 6, bins], scalars {field: int64 [ngroups]}) of trials given as rows [slots, 6 sectors, 6 series]."""
    n = len(rows_list)
    groups = list(range(n)) if groups is None else list(groups)
    ngroups = (max(groups) + 1 if groups else 0) if ngroups is None else ngroups
    series = np.zeros((6, ngroups, 6, bins), dtype=np.int64)
    sc = {f: np.zeros(ngroups, dtype=np.int64) for f in SCALARS}
    sc["tx_max"][:] = -1
    for rows, aT, g in zip(rows_list, access_times, groups):
        rows = np.asarray(rows, dtype=np.int64)
        sc["trials"][g] += 1
        sc["slots"][g] += len(rows)
        if not len(rows):
            continue
        for q, f in enumerate(SERIES):
            sc[f][g] += rows[..., q].sum()
        sc["tx_max"][g] = max(sc["tx_max"][g], rows[..., TX].max())
        b = (np.arange(len(rows), dtype=np.int64) * aT) // bin_ms
        inside = b < bins
        sc["overflow_tx"][g] += rows[~inside][..., TX].sum()
        for q in range(6):
            for c in range(6):
                np.add.at(series[q, g, c], b[inside], rows[inside, c, q])
    return series, sc


def same(tr, series, sc, mask_series=None):
    """A package NomaTrace against (series, scalars) of rebin; mask_series: a bool array broadcastable to the series, False where the reference is unknown."""
    got = tr.series.astype(np.int64)
    ok = np.array_equal(got, series) if mask_series is None else bool(((got == series) | ~mask_series).all())
    return ok and all(np.array_equal(tr.scalars[f], sc[f]) for f in SCALARS if mask_series is None or f not in ("tx", "used", "overflow_tx", "tx_max"))
