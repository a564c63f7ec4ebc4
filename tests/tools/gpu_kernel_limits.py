"""The limit table on the GPU (tests/tools/kernel_limits.py): every kernel-selection limit of the engine from both sides, judged by the oracle.
usage: [PRACH_LIB=…/libprach_hip.so] gpu_kernel_limits.py [CASE or LIMIT …]

Every case is a call of its own with the case's engine options: the trial against the oracle with tests/test_gpu_parity.py's assert_same bar (every
KEYS counter, totalDelay, all 16 logged fields of every UE; NOMA.c as tests/test_noma.py), the call's prach_timing against the pin the engine's source
predicts for that side of the limit (rec_mode, cluster_size, fallback_trials == 0, trial_kernel_reruns == 0); a case past a limit of the library itself
must return PRACH_ERR_UNSUPPORTED.  One GPU process, no retries: a call that fails with another status ends the run.  Prints a line per case with the
observed pin, then `done N cases B bad`; exit status 1 if B > 0 or the run ended early."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gpu_kernel_matrix as gkm  # (the oracle call, the comparison and the package of the kernel matrix's runner)
from kernel_limits import CASES, LEAVES, MIXED_CALL, OPT_DEFAULTS

pkg, ob = gkm.pkg, gkm.ob
ERR_UNSUPPORTED = -2  # include/prach.h
PIN_FIELDS = ("rec_mode", "cluster_size", "fallback_trials", "trial_kernel_reruns", "launches")


def trial_of(case):
    """gpu_kernel_matrix's trial tuple (program, variant, nUE, overrides, rng, seed)."""
    return ("noma" if case["variant"] == 2 else "beta", case["variant"], case["nUE"], case["kw"], case["rng"], case["seed"])


def set_opts(eng, opts):
    for k, v in OPT_DEFAULTS.items():
        eng.set(k, v)
    for k, v in opts.items():
        eng.set(k, v)


def pin_text(tm):
    return " ".join(f"{k}={getattr(tm, k)}" for k in PIN_FIELDS)


def main(names):
    mixed = dict(MIXED_CALL, trials=[("beta", v, n, kw, MIXED_CALL["rng"], s) for v, n, kw, s in MIXED_CALL["trials"]])
    cases = [c for c in CASES if not names or c["name"] in names or c["limit"] in names]
    with_mixed = not names or mixed["name"] in names or mixed["limit"] in names
    assert cases or with_mixed, f"no case or limit named {names}"
    t0 = time.time()
    todo = {gkm.key(trial_of(c)): trial_of(c) for c in cases if c["expect"] == "exact"}
    if with_mixed:
        todo.update({gkm.key(t): t for t in mixed["trials"]})
    ob.lib()
    nth = max(1, min(8, int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)))
    order = sorted(todo, key=lambda k: -todo[k][2] * (todo[k][3].get("max_steps") or 10000))  # (longest first)
    with ThreadPoolExecutor(max_workers=nth) as ex:
        ref = dict(zip(order, ex.map(gkm.oracle, [todo[k] for k in order])))
    print(f"oracle: {len(ref)} distinct trials in {time.time() - t0:.1f} s ({nth} threads)  library {os.path.basename(pkg.LIB_PATH)}", flush=True)
    eng = pkg.Engine(0)
    total = nbad = 0
    ended = None
    for c in cases:
        total += 1
        set_opts(eng, c["opts"])
        t = trial_of(c)
        cfg = pkg.make_cfg(c["nUE"], variant=c["variant"], rng_mode=c["rng"], seed=c["seed"], **c["kw"])
        head = f"case {c['name']:<26} {c['limit']:<20} {c['side']:<3}"
        t1 = time.time()
        try:
            (res,), (logs,) = eng.run_trials([cfg], want_logs=True)
        except pkg.PrachError as e:
            if c["expect"] == "unsupported" and e.status == ERR_UNSUPPORTED:
                print(f"{head} ok  status={e.status} (PRACH_ERR_UNSUPPORTED, as expected)", flush=True)
                continue
            nbad += 1
            print(f"{head} BAD the call failed: {e}", flush=True)
            ended = c["name"]
            break
        tm = eng.timing()
        why = []
        if c["expect"] == "unsupported":
            why.append("the call succeeded, PRACH_ERR_UNSUPPORTED expected")
        else:
            got = {k: getattr(tm, k) for k in c["pin"]}
            if got != c["pin"]:
                why.append(f"NOT PINNED: the table expects {c['pin']}")
            bad, _ = gkm.compare(t, res, logs, ref[gkm.key(t)])  # (the routes of one limit share a trial)
            if bad:
                why.append(f"MISMATCH {bad}")
        excused = c["name"] in LEAVES and len(why) == 1 and why[0].startswith("NOT PINNED")  # (left its kernel by a capacity, as listed: exact all the same)
        if excused:
            why = []
        elif why:
            nbad += 1
        print(f"{head} {'BAD' if why else 'ok '} {'(leaves: ' + LEAVES[c['name']] + ') ' if excused else ''}{pin_text(tm)} steps={res.steps} success={res.nSuccessUE} kernel={tm.kernel_ms:.1f}ms wall={time.time() - t1:.2f}s"
              + "".join(f"\n    {w}" for w in why), flush=True)
        del logs
    if with_mixed and ended is None:
        total += 1
        set_opts(eng, mixed["opts"])
        head = f"case {mixed['name']:<26} {mixed['limit']:<20} mix"
        cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s, **kw) for _, v, n, kw, r, s in mixed["trials"]]
        try:
            res, logs = eng.run_trials(cfgs, want_logs=True)
            tm = eng.timing()
            why = []
            got = {k: getattr(tm, k) for k in mixed["pin"]}
            if got != mixed["pin"]:
                why.append(f"NOT PINNED: the table expects {mixed['pin']}")
            for t, rs_, lg in zip(mixed["trials"], res, logs):
                bad, _ = gkm.compare(t, rs_, lg, ref[gkm.key(t)])
                if bad:
                    why.append(f"MISMATCH {t[1:]}: {bad}")
            nbad += bool(why)
            print(f"{head} {'BAD' if why else 'ok '} {pin_text(tm)} trials={len(cfgs)} kernel={tm.kernel_ms:.1f}ms" + "".join(f"\n    {w}" for w in why), flush=True)
        except pkg.PrachError as e:
            nbad += 1
            ended = mixed["name"]
            print(f"{head} BAD the call failed: {e}", flush=True)
    if ended is None:
        set_opts(eng, {})
        eng.close()
    else:
        print(f"run ended at {ended}: nothing more is started on the device after a failed call", flush=True)
    print(f"done {total} cases {nbad} bad ({time.time() - t0:.1f} s)" + (" ENDED EARLY" if ended else ""), flush=True)
    return 1 if nbad or ended else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
