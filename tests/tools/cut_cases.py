"""The cut sweep: every simulation kernel, pinned by engine options, stopped at consecutive subframes (max_steps = c) and judged by an oracle run cut at the same c.

Every kernel keeps per-UE state lazily and rebuilds the logged record when the trial ends, and the last subframe of a stopped trial takes paths of its
own (prach_lcluster.hip: `ahead`, `defer`, the epilogue; prach_cluster.hip: `ahead`; prach_noma.hip: has_next, tend_slot; prach_batch.hip: events still
on a calendar list).  What a stopped trial looks like depends on the subframe it is stopped in, so the same few base trials are run once per cut, for
runs of CONSECUTIVE cuts: a kernel that agrees with the oracle at c and not at c + 1 is wrong in subframe c or in its epilogue.

tests/tools/gpu_cut_sweep.py runs the rows on the GPU (tests/test_gpu_cut_sweep.py, one child process per row); tests/test_cut_cases_cpu.py proves
without a GPU, from the oracle alone, that the cuts contain what they are there for (check_* below).  Plain data, a generator and those checks: no GPU,
no package import.  The generator is deterministic (fixed seeds, no clock) and writes nothing: the cases are rebuilt from the oracle each time.

The oracle's grant count, restated from prach_oracle.c (preambleCollision and the head of the subframe loop): grantCheck is set to 0 in every subframe
with time % 5 == 0 (a literal 5, not accessTime); every singleton call (a preamble that exactly one UE transmits in the subframe) adds 1 to it FIRST and
is granted if the count is then still below nGrantUL, so nGrantUL - 1 singletons are granted per window of 5 subframes and nGrantUL = 1 grants nobody."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import binding as ob
from kernel_matrix import BETA_CASES, ROWS
import trace_ref

# ---- rows ---------------------------------------------------------------------------------------------------------------------------------------------
# kernel_matrix.ROWS as they are, and the instantiations that matrix leaves out because they have no compiler-chosen v_bitop3 table.  A row here may add:
#   force      overrides laid over every base of the row (what keeps the call off another kernel by a LIMIT where no engine option does)
#   pipeline   (0, 1): the row runs once per value of the engine option (prach_cluster.hip: `ahead = pipelined && t + 1 < P.stop`)
# The pins are what choose_kernel (prach_engine.hip) predicts:
#   cluster=4, lds_records=0, Philox   lslots = 0, not compact (G > 1)            -> CLUSTER_REC_G16 (0), cluster_kernel<false, 0>
#   cluster=4, fast=0, Philox          lslots > 0, use_fast_kernel false          -> CLUSTER_REC_L16 (2), cluster_kernel<false, 2>
#   cluster=1, glibc, maxRarWindow=12  batch_eligible false (batch_max_rar_window() = 11), compact: 10 000 + backoff + accessTime + 64 < 63 000
#                                                                                 -> CLUSTER_REC_H8 (1), cluster_kernel<true, 1>  (kernel_limits.py: batch_rar12_glibc)
#   legacy=1, glibc                    run_trials_impl: every trial on trial_kernel (cluster_size 0), trial_kernel<true>
#   noma_host_activation=1, glibc      run_noma_glibc: noma_glibc_slot_loop, one noma_glibc_slot_kernel launch per access slot (no cluster launch: cluster_size 0)
NEW_ROWS = [
    dict(name="cluster4_global_philox", kernels=["cluster_kernel<false, 0>"], program="beta", rng=1,
         opts=dict(cluster=4, lds_records=0), pin=dict(rec_mode=0, cluster_size=4)),
    dict(name="cluster4_lds_philox", kernels=["cluster_kernel<false, 2>"], program="beta", rng=1,
         opts=dict(cluster=4, fast=0), pin=dict(rec_mode=2, cluster_size=4)),
    dict(name="cluster_compact_glibc", kernels=["cluster_kernel<true, 1>"], program="beta", rng=0,
         opts=dict(cluster=1), pin=dict(rec_mode=1, cluster_size=1), force=dict(maxRarWindow=12)),
    dict(name="legacy_glibc", kernels=["trial_kernel<true>"], program="beta", rng=0,
         opts=dict(legacy=1), pin=dict(cluster_size=0)),
    dict(name="noma_glibc_slots", kernels=["noma_glibc_slot_kernel", "noma_glibc_finish_kernel"], program="noma", rng=0,
         opts=dict(noma_host_activation=1), pin=dict(cluster_size=0)),
]
CUT_ROWS = [dict(r) for r in ROWS] + NEW_ROWS
for _r in CUT_ROWS:
    if any(k.startswith("cluster_kernel<") for k in _r["kernels"]):
        _r["pipeline"] = (1, 0)
ROW = {r["name"]: r for r in CUT_ROWS}

# every engine option a row sets, at the engine's defaults
OPT_DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0, fast=1, lds_records=1, pipeline=1, noma_host_activation=0)

# Trials per call.  The workgroups of a cluster wait for each other, so the engine halves the cluster size of a call until all its clusters are resident
# (prach_engine.hip cluster_size: G x trials <= resident_limit, 256 on the MI355X) and packs lean clusters on XCDs only while ((m + 7) / 8) x G <= 32: a
# row's pin holds for calls of at most 128 workgroups.  One workgroup per trial: every trial of the row in calls of up to 512.
def trials_per_call(row):
    g = row["pin"].get("cluster_size", 0)
    return max(1, 128 // g) if g > 1 else 512


# kernels of the library that no row runs, by what they are (tests/test_cut_cases_cpu.py: every other symbol must be pinned by a row)
LEFT_OUT = dict(
    reducers=["columns_kernel", "dist_kernel", "noma_census_kernel", "noma_columns_kernel", "noma_pick_kernel", "noma_summary_kernel", "pick_kernel",
              "sojourn_kernel", "summary_kernel", "timeline_kernel", "trace_kernel", "xtab_kernel"],
    stream=["glibc_stream_jobs_kernel", "glibc_stream_kernel"],
    activation=[],  # (noma_activation_kernel runs in front of every noma_kernel launch of the noma*_philox rows; the matrix names it, and so do these rows)
)

# ---- base trials --------------------------------------------------------------------------------------------------------------------------------------
# Beta.c / RandomAccessWithNOMA: (name, nUE, overrides), each for both variants; a row runs them in its own RNG mode, seed 700 + 10 k + variant.
_CORNER = dict([(n, (u, kw)) for n, u, kw in BETA_CASES])["corner_1500"]
BETA_BASES = [
    ("default_1500", 1500, {}),
    ("at7_g3_2500", 2500, dict(accessTime=7, nGrantUL=3, nPreamble=20, backoff=10)),
    ("at2_g3_2000", 2000, dict(accessTime=2, nGrantUL=3, nPreamble=16)),
    ("corner_1500", _CORNER[0], dict(_CORNER[1])),  # nGrantUL = 1: no grant ever, a call without a grant left in every calling subframe
    ("default_64", 64, {}),                         # every UE succeeds: the loop breaks at nSuccessUE == nUE (Beta.c:180)
]
# NOMA.c: (name, nUE, seed, overrides: the engine's names), after kernel_matrix.NOMA_CASES at reduced nUE
NOMA_BASES = [
    ("noma_1500", 1500, 0, {}),
    ("noma_at3_2000", 2000, 9, dict(maxRarWindow=7, accessTime=3, nGrantUL=3)),
    ("noma_64", 64, 14, dict(nGrantUL=30)),  # every UE is served in both RNG modes (seed 14): NOMA.c:707-710 breaks behind the last success
    ("noma_g1_1500", 1500, 11, dict(nGrantUL=1, maxMsg2TxCount=0, maxRarWindow=1, nPreamble=2)),
]
# Base trials that leave a row's kernel by design (as kernel_matrix.LEAVES: a per-subframe capacity of the kernel exceeded, the trial rerun exactly on the
# next kernel of the engine's ladder): base name -> {row name: (part, reason)}, part "all" (the base is not run for that row) or the part of its cuts
# that is not ("head", "busy", "tail").  Measured on the MI355X with gpu_cut_sweep.py, which names the cuts at which a base leaves; every other cut of every
# base stays on its row's kernel, or the sweep fails.
_SATURATED = ("tail", "16 preambles and 2 grants per 5 subframes for 2000 UEs: from about subframe 2500 on every preamble collides in every subframe and nobody is "
              "granted again.  Run to the end, such a trial uses up the chunk pool of the 1024-thread batch kernel's calendar at subframe 4174 (PRACH_VERBOSE: capacity "
              "9), is rerun with lists of nUE entries (a fallback trial), uses that pool up at subframe 7312 and goes to trial_kernel (as kernel_matrix.LEAVES: "
              "p3_b40_at6).  Head and busy window, before subframe 1600, stay")
LEAVES = {
    "at2_g3_2000": {"batch_w16_philox": _SATURATED, "batch_glibc": _SATURATED},
}

MAX_TIME = 10000  # (no base has Uniform arrivals)
BUSY = 64


def bases_of(row):
    """[(base name, trial without a cut)] of a row: trials are gpu_kernel_matrix's tuples (program, variant, nUE, overrides, rng, seed)."""
    r, force = row["rng"], row.get("force", {})
    if row["program"] == "noma":
        out = [(name, ("noma", 2, n, dict(kw, **force), r, s)) for name, n, s, kw in NOMA_BASES]
    else:
        out = [(f"{name}_v{v}", ("beta", v, n, dict(kw, **force), r, 700 + 10 * k + v)) for k, (name, n, kw) in enumerate(BETA_BASES) for v in (0, 1)]
    return [(name, t) for name, t in out if left_part(row, name) != "all"]


def left_part(row, name):
    """The part of a base's cuts that leaves the row's kernel by design: None, "all", "head", "busy" or "tail"."""
    return LEAVES.get(name.rsplit("_v", 1)[0] if row["program"] == "beta" else name, {}).get(row["name"], (None, ""))[0]


def key(t):
    return (t[0], t[1], t[2], tuple(sorted(t[3].items())), t[4], t[5])


def with_cut(t, c):
    return (t[0], t[1], t[2], dict(t[3], max_steps=int(c)), t[4], t[5])


def noma_cfg(n, kw):
    """The oracle's NOMA.c configuration of overrides under the engine's names (maxMsg2TxCount is NOMA.c's maxMsg1ReTx)."""
    okw = dict(kw)
    if "maxMsg2TxCount" in okw:
        okw["maxMsg1ReTx"] = okw.pop("maxMsg2TxCount")
    return ob.make_noma_cfg(n, **okw)


def oracle(t):
    """(ocfg or None, (result, UE log)) of one trial: what gpu_kernel_matrix.compare takes."""
    prog, v, n, kw, r, s = t
    if prog == "noma":
        ocfg = noma_cfg(n, kw)
        return ocfg, ob.noma_run_trial(ocfg, ob.Rng(r, s))
    return None, ob.run_trial(ob.make_cfg(n, variant=v, **kw), ob.Rng(r, s))


_ref = {}


def oracle_many(trials, threads=None):
    """{key: oracle(trial)} of the distinct trials, on a pool of at most 16 threads (plain C behind ctypes, no global state while the census hook is
    off).  Cached for the process."""
    todo = {}
    for t in trials:
        if key(t) not in _ref:
            todo.setdefault(key(t), t)
    if todo:
        ob.lib()
        nth = threads or max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)))
        order = sorted(todo, key=lambda k: -todo[k][2] * todo[k][3].get("max_steps", MAX_TIME))  # (longest first)
        with ThreadPoolExecutor(max_workers=nth) as ex:
            _ref.update(zip(order, ex.map(oracle, [todo[k] for k in order])))
    return {key(t): _ref[key(t)] for t in trials}


# ---- the uncut run of a base: census and cuts (single-threaded: the census hook is process-wide) ------------------------------------------------------
_uncut = {}


def grants_of(t):
    kw = t[3]
    return kw.get("nGrantUL", 54 if t[1] == 0 else 12)  # (prach_cfg_defaults: Beta.c:49 / WithNOMA:73)


def kinds(calls, singles, nGrantUL):
    """Per subframe t, what kind of LAST subframe t is: 'grant' a singleton call finds an UL grant left in its 5-subframe window (a grant is written in the
    last subframe: only the epilogue can apply it); 'nogrant' calls, none of them granted; 'quiet' no call at all.  Boolean arrays."""
    n = len(calls)
    cs = np.concatenate([[0], np.cumsum(singles)])
    t = np.arange(n)
    before = cs[t] - cs[t - t % 5]  # grantCheck at the head of subframe t
    grant = (singles > 0) & (before + 1 < nGrantUL)
    return dict(grant=grant, nogrant=(calls > 0) & ~grant, quiet=calls == 0)


def uncut(t):
    """The uncut oracle run of a base: dict(res, steps, early, calls, singles (Beta.c / WithNOMA), cuts=dict(head, busy, tail))."""
    k = key(t)
    if k in _uncut:
        return _uncut[k]
    prog, v, n, kw, r, s = t
    aT = kw.get("accessTime", 5)
    u = dict(aT=aT)
    if prog == "noma":
        res, sectors = ob.noma_run_trial_traced(noma_cfg(n, kw), ob.Rng(r, s))
        per_slot = np.bincount([x["slot"] for x in sectors], minlength=1)
        peak = int(np.argmax(per_slot)) * aT  # the subframe with the most resolved sectors (the first of them)
    else:
        calls, singles, res = trace_ref.census((v, n, kw, r, s))
        u.update(calls=calls, singles=singles)
    steps, X = int(res.steps), int(res.time_exit)
    early = steps == X + 1  # the loop broke in subframe X (prach_oracle.h: steps == time_exit, + 1 when the loop broke early)
    assert early or steps == X == MAX_TIME
    head = list(range(1, 4 * max(aT, 5) + 1))
    tail = list(range(X - 2, X + 4)) if early else list(range(MAX_TIME - 2, MAX_TIME + 2))
    last = steps - 1  # the last subframe the uncut run executes
    if prog == "noma":
        lo = peak - BUSY // 2
    else:
        kd = kinds(calls, singles, grants_of(t))
        cnt = {q: np.concatenate([[0], np.cumsum(a)]) for q, a in kd.items()}
        cc = np.concatenate([[0], np.cumsum(calls)])
        starts = np.arange(min(len(head), max(0, steps - BUSY)), max(1, steps - BUSY + 1))  # (behind the head, where the trial is long enough)
        per = np.sort([cnt[q][np.minimum(starts + BUSY, steps)] - cnt[q][starts] for q in ("grant", "nogrant", "quiet")], axis=0)
        load = cc[np.minimum(starts + BUSY, steps)] - cc[starts]
        best = np.lexsort((starts, -load, -per[1], -per[0]))[0]  # the most of the rarest kind, of the second rarest, the most calls, the earliest
        lo = int(starts[best])
    lo = max(0, min(lo, last + 1 - BUSY))
    busy = [x + 1 for x in range(lo, lo + BUSY) if 0 <= x <= last]  # last subframes lo .. lo + 63
    u.update(res=res, steps=steps, X=X, early=early, cuts=dict(head=head, busy=busy, tail=[c for c in tail if c >= 1]))
    _uncut[k] = u
    return u


def cuts_of(t, without=None):
    c = uncut(t)["cuts"]
    return sorted(set().union(*[c[part] for part in ("head", "busy", "tail") if part != without]))


def trials_of(row):
    """[(base name, base trial, cut, the trial cut there)] of a row."""
    return [(name, t, c, with_cut(t, c)) for name, t in bases_of(row) for c in cuts_of(t, left_part(row, name))]


# ---- the CPU-side checks (tests/test_cut_cases_cpu.py): lists of failure texts ------------------------------------------------------------------------
def check_rows():
    """Row table: names unique, at least two bases per variant after LEAVES, every general cluster_kernel row with the pipeline both ways."""
    bad = []
    if len(ROW) != len(CUT_ROWS):
        bad.append("row names are not unique")
    if [{k: x for k, x in c.items() if k != "pipeline"} for c in CUT_ROWS[:len(ROWS)]] != ROWS:
        bad.append("CUT_ROWS does not start with kernel_matrix.ROWS as they are")
    for row in CUT_ROWS:
        per = {}
        for name, t in bases_of(row):
            per[t[1]] = per.get(t[1], 0) + 1
        want = (2,) if row["program"] == "noma" else (0, 1)
        if any(per.get(v, 0) < 2 for v in want):
            bad.append(f"{row['name']}: fewer than two base trials of a variant: {per}")
        if any(k.startswith("cluster_kernel<") for k in row["kernels"]) and sorted(row.get("pipeline", ())) != [0, 1]:
            bad.append(f"{row['name']}: a general cluster_kernel row without pipeline on and off")
        if set(row["opts"]) - set(OPT_DEFAULTS):
            bad.append(f"{row['name']}: option without a default in OPT_DEFAULTS: {set(row['opts']) - set(OPT_DEFAULTS)}")
    return bad


def check_symbols(symbols):
    """Every kernel symbol of the built library (scripts/isa_bitop3.py's names) is pinned by a row or listed in LEFT_OUT, and the rows name none it has not."""
    pinned = {k for r in CUT_ROWS for k in r["kernels"]}
    left = [p for names in LEFT_OUT.values() for p in names]
    bad = [f"no row of CUT_ROWS pins the simulation kernel {s}" for s in sorted(symbols) if s not in pinned and s.split("<")[0] not in left]
    bad += [f"CUT_ROWS names a kernel the library does not have: {k}" for k in sorted(pinned - set(symbols))]
    bad += [f"LEFT_OUT names a kernel the library does not have: {p}" for p in left if not any(s.split("<")[0] == p for s in symbols)]
    return bad


def log_of(oc):
    """The 16 int32 fields of every UE of an oracle run (Beta.c / WithNOMA: ob.UE_FIELDS; NOMA.c: ob.NOMA_UE_FIELDS without the gain)."""
    ues = oc[1][1]
    if oc[0] is not None:
        return np.frombuffer(ues, dtype=np.dtype([("i", np.int32, 16), ("g", np.float64)]))["i"]
    return np.frombuffer(ues, dtype=np.int32).reshape(-1, 16)


def result_bytes(oc):
    return bytes(oc[1][0]) + log_of(oc).tobytes()


_F = {n: i for i, n in enumerate(ob.UE_FIELDS)}


def check_base(t):
    """One base against its uncut run: (failure texts, facts).  facts: how often each kind of last subframe occurs among its cuts, and which of the
    logged states the oracle's logs at the cuts contain."""
    prog, v, n, kw, r, s = t
    u, cuts = uncut(t), cuts_of(t)
    ref = oracle_many([t] + [with_cut(t, c) for c in cuts])
    whole = ref[key(t)]
    bad, facts = [], dict(cuts={}, active=set(), passes=set())  # cuts: {cut: the kind of its last subframe and the logged states seen there}
    aT, steps, X = u["aT"], u["steps"], u["X"]
    lasts = {c - 1 for c in cuts if c <= steps}
    for m in sorted({aT, 5}):
        if {x % m for x in lasts} != set(range(m)):
            bad.append(f"the last subframes of the cuts miss a residue of {m}")
    if min(cuts) != 1 or cuts[:4 * max(aT, 5)] != list(range(1, 4 * max(aT, 5) + 1)) or len(u["cuts"]["busy"]) != BUSY:
        bad.append(f"head 1..{4 * max(aT, 5)} or the busy window of {BUSY} consecutive cuts is incomplete")
    # tail: a cut at or behind the end of the trial IS the uncut trial; around an early exit, steps and time_exit as prach_oracle.h describes them
    for c in cuts:
        res = ref[key(with_cut(t, c))][1][0]
        want = (min(c, X), min(c, steps))
        if (int(res.time_exit), int(res.steps)) != want:
            bad.append(f"cut {c}: time_exit, steps = {res.time_exit}, {res.steps}, expected {want}")
        if c >= (steps if u["early"] else MAX_TIME) and result_bytes(ref[key(with_cut(t, c))]) != result_bytes(whole):
            bad.append(f"cut {c} is at or behind the end of the trial and differs from the uncut run")
    need = [X - 1, X, X + 1, X + 2] if u["early"] else [MAX_TIME - 1, MAX_TIME, MAX_TIME + 1]
    if not set(need) <= set(cuts):
        bad.append(f"the tail misses one of the cuts {need}")
    if u["early"] and not (int(whole[1][0].nSuccessUE) == n and steps == X + 1):
        bad.append("an early exit without every UE successful")
    # prefix properties
    draws = [int(ref[key(with_cut(t, c))][1][0].draws) for c in cuts]
    if any(b < a for a, b in zip(draws, draws[1:])) or draws[-1] != int(whole[1][0].draws):
        bad.append("draws is not non-decreasing in the cut")
    if prog == "noma":
        for c in cuts:
            a = log_of(ref[key(with_cut(t, c))])
            facts["active"] |= set(np.unique(a[:, 2]).tolist())
        return bad, facts
    calls, singles = u["calls"], u["singles"]
    cs, cc = np.cumsum(singles), np.cumsum(calls)
    kd = kinds(calls, singles, grants_of(t))
    for c in cuts:
        oc = ref[key(with_cut(t, c))]
        res, a = oc[1][0], log_of(oc)
        e = min(c, steps)
        x, q = int(res.totalPreambleTxop), int(res.collisionPreambles)
        # (a single adds 1 to totalPreambleTxop only, a collided call the same amount to both: 1 in Beta.c, the number of colliding UEs in WithNOMA)
        if x - q != cs[e - 1] or (v == 0 and x != cc[e - 1]) or x < cc[e - 1] or q < cc[e - 1] - cs[e - 1] or int(res.collisionCalls) != cc[e - 1]:
            bad.append(f"cut {c}: totalPreambleTxop {x} / collisionPreambles {q} are not the census's sums over [0, {e})")
        facts["active"] |= set(np.unique(a[:, _F["active"]]).tolist())
        facts["cuts"][c] = dict(
            kind=[name for name in ("grant", "nogrant", "quiet") if kd[name][c - 1]][0] if c <= steps else None,
            backoff=bool((a[:, _F["nowBackoff"]] > 0).any()),
            rar=bool(((a[:, _F["rarWindow"]] > 0) & (a[:, _F["rarWindow"]] < kw.get("maxRarWindow", 6))).any()),
            msg2=bool(((a[:, _F["msg2Flag"]] == 1) & (a[:, _F["msg4Flag"]] == 0)).any()),
            fail=bool((a[:, _F["failCount"]] > 0).any()))
    # Every value of `active` the uncut run ever passes through: every UE starts at -1 and is 1 from its arrival on; 2 (granted) only ever turns into 0
    # (Msg4) or back into 1, so the values of the final log, -1 and 1 once anybody arrived, and 2 wherever the final log holds a 0 are all of them — except
    # a 2 that every UE has left again without one success, which no base here does (each has successes or, with nGrantUL = 1, no grant at all).
    final = set(np.unique(log_of(whole)[:, _F["active"]]).tolist())
    facts["passes"] = final | {-1} | ({1} if int(whole[1][0].activeCheck) > 0 else set()) | ({2} if 0 in final else set())
    if not facts["passes"] <= facts["active"]:
        bad.append(f"the logs at the cuts never show active = {sorted(facts['passes'] - facts['active'])}")
    return bad, facts


def check_row(row, facts):
    """Across the cuts a row runs (facts: {base name: check_base's facts}): every kind of last subframe at least 8 times, every logged state seen."""
    if row["program"] == "noma":
        return []
    bad = []
    mine = [(t[1], facts[name]["cuts"][c]) for name, t, c, _ in trials_of(row)]
    for kind in ("grant", "nogrant", "quiet"):
        n = sum(f["kind"] == kind for _, f in mine)
        if n < 8:
            bad.append(f"{row['name']}: only {n} cuts whose last subframe is of kind '{kind}'")
    for state, what in (("backoff", "nowBackoff > 0"), ("rar", "0 < rarWindow < maxRarWindow"), ("msg2", "msg2Flag == 1 and msg4Flag == 0")):
        if not any(f[state] for _, f in mine):
            bad.append(f"{row['name']}: no log at a cut has a UE with {what}")
    if not any(f["fail"] for v, f in mine if v == 1):
        bad.append(f"{row['name']}: no WithNOMA log at a cut has a UE with failCount > 0")
    return bad

