"""What the NOMA summary and the NOMA pick cost (prach_run_trials_noma_summary, prach_run_trials_noma_pick; csrc/prach_noma_select.hip), on NOMA.c's own
experiment (ten seeds x the ten sweep points 10 000 .. 100 000 UEs, Philox: 100 trials, 5.5 M UEs) and on one 100 000-UE trial.  Per workload, in ONE run,
medians of repeated calls after a warm-up call, the spread (max - min over the repetitions) beside the median; the calls (a), (b), (c), (p) and (e)
alternate inside every repetition, and (d) runs BEHIND them, in repetitions of its own (its 64 B per UE go to pageable host memory and would disturb the
calls next to it):
  (a) the summary call (the default: sojourn, timer, ptc, lost of the served at 500, 950, 990 permille): total_ms (the wall time of the call, which ends in a
      synchronise) and noma_summary_ms (HIP events around the kernel), and the kernel's byte floor: two passes of 48 B per UE (words 0-3 and 8-15) over 8 TB/s
  (b) the pick call `largest sojourn, k 16, served`: total_ms and noma_pick_ms; floor: three passes of 48 B per UE (classify, fine histogram, compaction)
  (c) the pick call `where state:5:5, who pending, by index, k 64` (the stranded UEs): one pass of 64 B per UE (STATE reads all four quarters)
  (p) the census call of the PARENT library (--parent DIR: the library built in that checkout, loaded next to this one; without it, this library's):
      noma_census_ms on the same input, the yardstick the issue names
  (e) plain prach_run_trials: kernel_ms of this library, of the parent, and of a SECOND copy of the parent (--parent2 DIR) — the parent's own spread against
      itself is the margin inside which this library's simulation kernels have to stay
  (d) the only route of the parent to the same answers: prach_run_trials with EVERY per-UE log plus the host definition (prach_noma_summary_from_logs /
      prach_noma_pick_from_logs of this library) — wall time, host part included.  The probe asserts that its results equal (a)'s and (b)'s
Prints markdown (profiles/noma_select_kernel.md is this output).
usage: gpu_noma_select_probe.py [--reps 5] [--parent DIR] [--parent2 DIR] [--workloads grid,single]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as g  # noqa: E402

HBM_BYTES_PER_MS = 8e9  # 8 TB/s
TOP = dict(where=(), order="largest", key="sojourn", k=16)
STRANDED = dict(where=[("state", 5, 5)], order="index", key=None, k=64)


def load_other(root, name):
    """The package of another checkout (its own library), under a module name of its own."""
    d = os.path.join(root, "5g-nr-randomaccess_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent2", default=None)
    ap.add_argument("--workloads", default="grid,single")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    par = load_other(args.parent, "nr_randomaccess_amd_parent") if args.parent else pkg
    par2 = load_other(args.parent2, "nr_randomaccess_amd_parent2") if args.parent2 else par
    peng = par.Engine(0) if args.parent else eng
    peng2 = par2.Engine(0) if args.parent2 else peng
    noma = lambda p, n, s: p.make_cfg(n, variant=p.VARIANT_NOMA_C, rng_mode=p.RNG_PHILOX, seed=s)
    work = {"grid": ("NOMA.c's experiment (10 seeds x 10 points, 5.5 M UEs)", lambda p: [noma(p, n, s) for s in range(10) for n in range(10000, 100001, 10000)]),
            "single": ("one 100 000-UE trial", lambda p: [noma(p, 100000, 0)])}
    med = statistics.median
    sp = lambda v, d=2: f"{med(v):.{d}f} ({max(v) - min(v):.{d}f})"
    served, pending = pkg.NOMA_WHO["served"], pkg.NOMA_WHO["pending"]
    print(f"census and plain calls (p), (e) of: {'--parent ' + args.parent if args.parent else 'this checkout'}; second copy: {args.parent2 or 'none'}; reps {args.reps}\n")
    print("| workload | (a) summary: total_ms (spread) | noma_summary_ms (spread) | floor (ms) | / floor | (b) pick top 16: total_ms (spread) | noma_pick_ms (spread) | floor (ms) | / floor | "
          "(c) pick stranded: total_ms (spread) | noma_pick_ms (spread) | floor (ms) | / floor | (p) parent census: noma_census_ms (spread) | (e) plain kernel_ms here (spread) | "
          "parent (spread) | parent, 2nd copy (spread) | plain total_ms here (spread) | (d) logs + host summary: ms (spread) | (d) / (a) | (d) logs + host pick: ms (spread) | (d) / (b) |")
    print("|" + "---|" * 22)
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, pcfgs, pcfgs2 = make(pkg), make(par), make(par2)
        groups = [k % 10 for k in range(len(cfgs))] if len(cfgs) > 1 else [0]
        nue = sum(c.nUE for c in cfgs)
        for e, cs in ((eng, cfgs), (peng, pcfgs), (peng2, pcfgs2)):  # warm-up: the arenas, the code objects
            e.run_trials(cs)
        eng.run_trials_noma_summary(cfgs)
        eng.run_trials_noma_pick(cfgs, who=served, **TOP)
        peng.run_trials_noma_census(pcfgs, groups=groups)
        a_tot, a_k, b_tot, b_k, c_tot, c_k, p_k, e_here, e_par, e_par2, e_tot, d_sm, d_pk = ([] for _ in range(13))
        for rep in range(args.reps):
            _, _, sm = eng.run_trials_noma_summary(cfgs)
            tm = eng.timing()
            a_tot.append(tm.total_ms); a_k.append(tm.noma_summary_ms)
            peng.run_trials(pcfgs)
            e_par.append(peng.timing().kernel_ms)
            _, _, pk = eng.run_trials_noma_pick(cfgs, who=served, **TOP)
            tm = eng.timing()
            b_tot.append(tm.total_ms); b_k.append(tm.noma_pick_ms)
            peng2.run_trials(pcfgs2)
            e_par2.append(peng2.timing().kernel_ms)
            eng.run_trials_noma_pick(cfgs, who=pending, **STRANDED)
            tm = eng.timing()
            c_tot.append(tm.total_ms); c_k.append(tm.noma_pick_ms)
            peng.run_trials_noma_census(pcfgs, groups=groups)
            p_k.append(peng.timing().noma_census_ms)
            eng.run_trials(cfgs)
            tm = eng.timing()
            e_here.append(tm.kernel_ms); e_tot.append(tm.total_ms)
        for rep in range(args.reps):  # (d), apart
            t0 = time.perf_counter()
            res, logs = peng.run_trials(pcfgs, want_logs=True)
            hsm = pkg.noma_summary_from_logs(cfgs, [r.steps for r in res], logs)
            d_sm.append(1e3 * (time.perf_counter() - t0))
            del logs
            t0 = time.perf_counter()
            res, logs = peng.run_trials(pcfgs, want_logs=True)
            hpk = pkg.noma_pick_from_logs(cfgs, [r.steps for r in res], logs, who=served, **TOP)
            d_pk.append(1e3 * (time.perf_counter() - t0))
            del logs
            assert sm.rows.tobytes() == hsm.rows.tobytes() and pk.same_as(hpk), "the two routes disagree"
        fa, fb, fc = 2 * 48 * nue / HBM_BYTES_PER_MS, 3 * 48 * nue / HBM_BYTES_PER_MS, 64 * nue / HBM_BYTES_PER_MS
        print(f"| {name} | {sp(a_tot)} | {sp(a_k, 3)} | {fa:.4f} | {med(a_k) / fa:.1f} | {sp(b_tot)} | {sp(b_k, 3)} | {fb:.4f} | {med(b_k) / fb:.1f} | {sp(c_tot)} | {sp(c_k, 3)} | {fc:.4f} | "
              f"{med(c_k) / fc:.1f} | {sp(p_k, 3)} | {sp(e_here)} | {sp(e_par)} | {sp(e_par2)} | {sp(e_tot)} | {sp(d_sm, 0)} | {med(d_sm) / med(a_tot):.1f} | {sp(d_pk, 0)} | "
              f"{med(d_pk) / med(b_tot):.1f} |", flush=True)

    # the findings on NOMA.c's seed 0, 3000 UEs, as the two calls print them
    c = noma(pkg, 3000, 0)
    _, _, sm = eng.run_trials_noma_summary([c], ("sojourn", "timer", "lost"), served, (500, 1000))
    _, _, pk = eng.run_trials_noma_pick([c], who=pending, **STRANDED)
    _, _, top = eng.run_trials_noma_pick([c], who=served, **TOP)
    r = sm.rows[0]
    print(f"\nNOMA.c seed 0, 3000 UEs, 10 000 subframes (Philox): served {int(r['served'])}, pending {int(r['pending'])}, restarted {int(r['restarted'])}; sojourn median "
          f"{int(r['q'][0][0])} ms, longest {int(r['q'][0][1])} ms; timer longest {int(r['q'][1][1])} ms")
    print(f"pick `state:5:5, pending`: matched {int(pk.headers['matched'][0])}, the first UEs {[int(v) for v in pk.rows[0]['idx'][:8]]}")
    print(f"pick `largest sojourn, k 16`: keys {[int(v) for v in top.rows[0]['key']]}, ties left out {int(top.headers['ties_left_out'][0])}")
    eng.close()


if __name__ == "__main__":
    main()
