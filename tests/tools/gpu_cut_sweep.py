"""The cut sweep on the GPU (tests/tools/cut_cases.py): every simulation kernel, pinned by engine options, stopped at consecutive subframes, every
stopped trial judged by an oracle run cut at the same subframe.
usage: gpu_cut_sweep.py [ROW …]                  the rows named (default: all of cut_cases.CUT_ROWS)
       gpu_cut_sweep.py --scan ROW BASE LO HI    one base of one row at every cut LO .. HI, whatever the generator chose for it
       gpu_cut_sweep.py --grant [ROW …]          the grant sweep (tests/tools/grant_cases.py): the rows of grant_cases.GRANT_ROWS over its bases, cut behind the
                                                 chosen subframes; a row runs once per cluster size its bases need, each with the pin predicted for it

One engine per run.  The oracle's prefix runs come first, on a pool of at most 16 threads, distinct trials shared between the rows.  Per row the engine
options are set and the row's base x cut trials run in calls of cut_cases.trials_per_call trials; after EVERY call prach_timing must show the row's
pin (rec_mode, cluster_size) with no fallback trial and no rerun on trial_kernel, so that a trial counts only if the kernel of its row produced it.
Every trial against the oracle with gpu_kernel_matrix.compare: tests/test_gpu_parity.py's assert_same bar (every KEYS counter — draws, steps and
time_exit among them —, the float totalDelay, all 16 logged fields of every UE) or tests/test_noma.py's for NOMA.c, here with `steps` in both RNG
modes; bit-exact.  For every (row, base) with a mismatch one line names the smallest failing cut, the largest passing cut below it and the first UE
that differs with both records: a kernel that is right at c and wrong at c + 1 is wrong in subframe c or in its epilogue.  Prints a line per row with
the case count, the bad count, a crc32 digest of the results and logs, and the wall time, then `done N cases B bad`; exit status 1 if B > 0.  A call
that fails ends the run at once: nothing more is launched."""
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np

import gpu_kernel_matrix as gkm  # (the comparison, the pin test and the package of the kernel matrix's runner)
import cut_cases as CC
from trace_ref import lib_overrides  # (the oracle's sector_grants is the library's PRACH_FLAG_SECTOR_GRANTS)

pkg, ob = gkm.pkg, gkm.ob
assert set(gkm.DEFAULTS.items()) <= set(CC.OPT_DEFAULTS.items())


def first_difference(t, res, logs, oc):
    """The first UE whose record differs, with both records (or the counters, if only they differ)."""
    a = np.frombuffer(logs, dtype=np.int32).reshape(-1, 16)
    b = CC.log_of(oc)
    d = np.where((a != b).any(axis=1))[0]
    if d.size:
        i = int(d[0])
        names = ob.NOMA_UE_FIELDS if t[0] == "noma" else ob.UE_FIELDS
        f = [names[j] for j in np.where(a[i] != b[i])[0]]
        return f"{d.size} UEs differ, first UE {i} in {f}: {a[i].tolist()} != oracle {b[i].tolist()}"
    return "every UE record equal, the counters differ"


def judge(t, res, logs, oc):
    why, blob = gkm.compare(t, res, logs, oc)
    if why is None and t[0] == "noma" and res.steps != oc[1][0].steps:  # (prach_engine.hip steps_of: NOMA.c:707-710 breaks behind the last success)
        why = f"steps {res.steps} != oracle {oc[1][0].steps}"
    return why, blob


def run_row(eng, row, trials, ref, pipeline):
    """One pass over a row's trials [(base name, base, cut, trial)].  Returns (bad: {(base, cut): text}, digest, calls, kernel ms); raises PrachError."""
    for k, v in CC.OPT_DEFAULTS.items():
        eng.set(k, v)
    for k, v in row["opts"].items():
        eng.set(k, v)
    if pipeline is not None:
        eng.set("pipeline", pipeline)
    per = CC.trials_per_call(row)
    bad, digest, calls, kms = {}, 0, 0, 0.0
    for lo in range(0, len(trials), per):
        grp = trials[lo:lo + per]
        cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s, **lib_overrides(kw)) for _, _, _, (_, v, n, kw, r, s) in grp]
        res, logs = eng.run_trials(cfgs, want_logs=True)
        tm = eng.timing()
        calls += 1
        kms += tm.kernel_ms
        pf = gkm.pin_failure(row, tm)
        if pf:
            print(f"  {row['name']}: NOT PINNED {pf} ({len(grp)} trials, first {grp[0][0]} cut {grp[0][2]})", flush=True)
            left = {}
            for name, _, c, t in grp:  # (which of them left the kernel: each alone, the smallest cut per base reported)
                if len(grp) > 1:
                    eng.run_trials([pkg.make_cfg(t[2], variant=t[1], rng_mode=t[4], seed=t[5], **lib_overrides(t[3]))])
                if len(grp) == 1 or gkm.pin_failure(row, eng.timing()):
                    bad[(name, c)] = f"left the row's kernel: {gkm.pin_failure(row, eng.timing())}"
                    left.setdefault(name, []).append(c)
            for name, cs in left.items():
                print(f"  {row['name']}:   {name} leaves at {len(cs)} cuts, the smallest {min(cs)}, the largest {max(cs)}", flush=True)
            if not left:
                bad.update({(name, c): "a call of many trials lost the pin, no trial alone did" for name, _, c, _ in grp})
        for (name, _, c, t), rs_, lg in zip(grp, res, logs):
            why, blob = judge(t, rs_, lg, ref[CC.key(t)])
            digest = zlib.crc32(blob, digest)
            if why:
                bad.setdefault((name, c), f"{first_difference(t, rs_, lg, ref[CC.key(t)])} | {' '.join(why.split())[:240]}")
        del res, logs
    return bad, digest, calls, kms


def report(row, tag, trials, bad):
    """Per base with a bad cut: the smallest failing cut, the largest passing cut below it, what differs there."""
    for name in dict.fromkeys(n for n, _ in bad):
        cuts = sorted(c for n, _, c, _ in trials if n == name)
        fails = sorted(c for n, c in bad if n == name)
        below = [c for c in cuts if c < fails[0]]
        print(f"  {row['name']}{tag} {name}: {len(fails)} of {len(cuts)} cuts bad; FIRST FAILING CUT {fails[0]}, largest passing cut below it "
              f"{below[-1] if below else 'none'}: {bad[(name, fails[0])]}", flush=True)


def main(argv):
    t0 = time.time()
    if argv[:1] == ["--scan"]:
        rname, bname, lo, hi = argv[1], argv[2], int(argv[3]), int(argv[4])
        row = CC.ROW[rname]
        base = dict(CC.bases_of(row))[bname]
        plan = [(row, [(bname, base, c, CC.with_cut(base, c)) for c in range(lo, hi + 1)])]
    elif argv[:1] == ["--grant"]:
        import grant_cases as GC
        unknown = [n for n in argv[1:] if n not in GC.GROW]
        assert not unknown, f"no grant row named {unknown}"
        plan = []
        for r in GC.GRANT_ROWS:
            if argv[1:] and r["name"] not in argv[1:]:
                continue
            per = {}  # (the row as sized for its trials' cluster size -> its trials)
            for srow, tag, base, c, t in GC.trials_of(r):
                g = srow["pin"]["cluster_size"]
                per.setdefault(g, (dict(srow, label=f"[cluster={g}]" if g > 1 else ""), []))[1].append((tag, base, c, t))
            plan += list(per.values())
    else:
        unknown = [n for n in argv if n not in CC.ROW]
        assert not unknown, f"no row named {unknown}"
        plan = [(r, CC.trials_of(r)) for r in CC.CUT_ROWS if not argv or r["name"] in argv]
    ref = CC.oracle_many([t for _, trials in plan for _, _, _, t in trials])
    print(f"oracle: {len(ref)} distinct trials in {time.time() - t0:.1f} s  library {os.path.basename(pkg.LIB_PATH)}", flush=True)
    eng = pkg.Engine(0)
    total = nbad = 0
    for row, trials in plan:
        for pipeline in row.get("pipeline", (None,)):
            tag = row.get("label", "") + ("" if pipeline is None else f"[pipeline={pipeline}]")
            t1 = time.time()
            try:
                bad, digest, calls, kms = run_row(eng, row, trials, ref, pipeline)
            except pkg.PrachError as e:
                print(f"  {row['name']}{tag}: a call failed: {e}\nrun ended: nothing more is started on the device after a failed call", flush=True)
                return 1
            report(row, tag, trials, bad)
            total += len(trials)
            nbad += len(bad)
            print(f"row {row['name'] + tag:<36} {'+'.join(row['kernels']):<45} cases={len(trials):4d} calls={calls:3d} bad={len(bad)} digest={digest:08x} "
                  f"kernel={kms:.1f}ms wall={time.time() - t1:.2f}s", flush=True)
    for k, v in CC.OPT_DEFAULTS.items():
        eng.set(k, v)
    eng.close()
    print(f"done {total} cases {nbad} bad ({time.time() - t0:.1f} s)", flush=True)
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
