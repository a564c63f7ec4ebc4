"""The quiet-subframe path of prach::lcluster_kernel on the GPU (tests/tools/quiet_cases.py): one base trial, one variant, one RNG mode, one cluster
size — uncut, stopped at the 64 consecutive subframes from the first one that has an off-slot singleton, and at the 64 from the first one that takes
the path (there subframes that take it and subframes that fall through to the general resolver alternate, and a stopped trial's epilogue needs the
last-caller table and the counters the path wrote).  Every trial against an oracle run cut at the same subframe through tests/test_gpu_parity.py's assert_same: every counter
and all 16 logged fields of every UE, bit-exact.  After EVERY call prach_timing must show the lean kernel (rec_mode 3) with no fallback trial and no
rerun on trial_kernel.
usage: gpu_lcluster_quiet.py BASE VARIANT RNG CLUSTER     prints `done N cases B bad`; exit status 1 if B > 0.  A call that fails ends the run."""
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import __graft_entry__ as g
import cut_cases as CC
import quiet_cases as QC

spec = importlib.util.spec_from_file_location("tgp", os.path.join(ROOT, "tests", "test_gpu_parity.py"))
tgp = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tgp)
pkg = g.load_package()


def main(argv):
    t0 = time.time()
    name, v, rng, G = argv[0], int(argv[1]), int(argv[2]), int(argv[3])
    case = QC.trial(name, v, rng)
    _, n, kw, _, seed = case
    cuts = QC.all_cuts_of(case)
    base = ("beta", v, n, kw, rng, seed)
    trials = [(None, base)] + [(c, CC.with_cut(base, c)) for c in cuts]
    ref = CC.oracle_many([t for _, t in trials])
    print(f"oracle: {len(ref)} trials in {time.time() - t0:.1f} s; cuts {cuts[0]} .. {cuts[-1]}", flush=True)
    eng = pkg.Engine(0)
    eng.set("cluster", G)
    per = max(1, 128 // G)  # (cut_cases.trials_per_call: the clusters of a call stay resident and packed up to 128 workgroups)
    bad = 0
    for lo in range(0, len(trials), per):
        grp = trials[lo:lo + per]
        try:
            res, logs = eng.run_trials([pkg.make_cfg(t[2], variant=t[1], rng_mode=t[4], seed=t[5], **t[3]) for _, t in grp], want_logs=True)
        except pkg.PrachError as e:
            print(f"a call failed: {e}\nrun ended: nothing more is started on the device after a failed call", flush=True)
            return 1
        tm = eng.timing()
        if not (tm.rec_mode == 3 and tm.fallback_trials == 0 and tm.trial_kernel_reruns == 0):
            bad += len(grp)
            print(f"NOT PINNED: rec_mode {tm.rec_mode} fallback_trials {tm.fallback_trials} trial_kernel_reruns {tm.trial_kernel_reruns} "
                  f"cluster_size {tm.cluster_size} (cuts {[c for c, _ in grp]})", flush=True)
            continue
        for (c, t), r_, lg in zip(grp, res, logs):
            ores, oues = ref[CC.key(t)][1]
            try:
                tgp.assert_same(pkg, r_, lg, ores, oues, (name, v, rng, G, c))
            except AssertionError as e:
                bad += 1
                print(f"cut {c}: {' '.join(str(e).split())[:500]}", flush=True)
    eng.set("cluster", 0)
    eng.close()
    print(f"done {len(trials)} cases {bad} bad ({time.time() - t0:.1f} s)", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
