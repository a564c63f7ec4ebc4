"""The exchange roles of prach::lcluster_kernel on the GPU (tests/tools/roles_cases.py): one case — a cluster size and a preamble count that make a
thread's second or third bucket role, the tail loop or the second event role live, or skip that role — with both variants in both RNG modes, each uncut
and stopped at a handful of subframes.  Every trial against an oracle run of the same trial through tests/test_gpu_parity.py's assert_same: every counter
and all 16 logged fields of every UE, bit-exact.  After EVERY call prach_timing must show the lean kernel (rec_mode 3) on a cluster of the case's size, with
no fallback trial and no rerun on trial_kernel.
usage: gpu_lcluster_roles.py CASE     prints `done N trials B bad`; exit status 1 if B > 0.  A call that fails ends the run."""
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
import roles_cases as RC

spec = importlib.util.spec_from_file_location("tgp", os.path.join(ROOT, "tests", "test_gpu_parity.py"))
tgp = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tgp)
pkg = g.load_package()


def main(argv):
    t0 = time.time()
    name = argv[0]
    G, n, kw = RC.CASE[name]
    trials = RC.trials(name)
    ref = CC.oracle_many([t for _, t in trials])
    print(f"{name}: G {G} nUE {n} {kw} live {RC.live(name)}; oracle: {len(ref)} trials in {time.time() - t0:.1f} s", flush=True)
    eng = pkg.Engine(0)
    eng.set("cluster", G)
    per = max(1, 128 // G)  # (cut_cases.trials_per_call: the clusters of a call stay resident)
    bad = 0
    # one variant and one RNG mode per call: a call is then one launch of one instantiation, and prach_timing speaks of all its trials
    for v, rng in ((0, 0), (0, 1), (1, 0), (1, 1)):
        mine = [(c, t) for c, t in trials if (t[1], t[4]) == (v, rng)]
        for lo in range(0, len(mine), per):
            grp = mine[lo:lo + per]
            try:
                res, logs = eng.run_trials([pkg.make_cfg(t[2], variant=t[1], rng_mode=t[4], seed=t[5], **t[3]) for _, t in grp], want_logs=True)
            except pkg.PrachError as e:
                print(f"a call failed: {e}\nrun ended: nothing more is started on the device after a failed call", flush=True)
                return 1
            tm = eng.timing()
            if not (tm.rec_mode == 3 and tm.cluster_size == G and tm.fallback_trials == 0 and tm.trial_kernel_reruns == 0):
                bad += len(grp)
                print(f"NOT PINNED: rec_mode {tm.rec_mode} cluster_size {tm.cluster_size} fallback_trials {tm.fallback_trials} trial_kernel_reruns "
                      f"{tm.trial_kernel_reruns} (rng {rng}, variants / cuts {[(t[1], c) for c, t in grp]})", flush=True)
                continue
            for (c, t), r_, lg in zip(grp, res, logs):
                ores, oues = ref[CC.key(t)][1]
                try:
                    tgp.assert_same(pkg, r_, lg, ores, oues, (name, t[1], rng, G, c))
                except AssertionError as e:
                    bad += 1
                    print(f"variant {t[1]} rng {rng} cut {c}: {' '.join(str(e).split())[:500]}", flush=True)
    eng.set("cluster", 0)
    eng.close()
    print(f"done {len(trials)} trials {bad} bad ({time.time() - t0:.1f} s)", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
