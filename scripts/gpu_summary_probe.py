"""What the per-trial summary costs (prach_run_trials_summary, csrc/prach_summary.hip), on the three workloads of DESIGN.md 4: the 1000-trial Beta.c grid,
BASELINE config 3 (the same grid of RandomAccessWithNOMA) and one 100 000-UE trial; levels 500, 950, 990.  Per workload, in ONE run, medians of repeated
calls after a warm-up call:
  (a) total_ms and timeline_ms of prach_run_trials_timeline (2002 bins of 5 ms, ten groups) on the same inputs: the timeline kernel reads the same log
      records once, the summary kernel twice, so timeline_ms is the yardstick.  With --parent DIR the timeline call is the one of the library built in
      that checkout (another commit), loaded next to this one; calls (a) and (b) alternate
  (b) total_ms and summary_ms of prach_run_trials_summary without host logs, per workgroup shape (engine option summary_threads), the spread (max - min
      over the repetitions) beside the median
  (c) on the grids, the only route of a library without the summary to per-trial sojourn percentiles: prach_run_trials_sojourn with one group per trial, ONE
      arrival row and 10 012 delay bins of 1 ms, plus prach_sojourn_quantile per trial and level — wall time, host extraction included.  The probe asserts
      that its medians equal level 500 of (b) (the one level at which the two rank rules coincide)
and, beside summary_ms, the kernel's byte floor: 2 passes x 48 B of the 64-byte record per UE (three 16-byte loads), over 8 TB/s.  Prints one markdown table
(profiles/summary_kernel.md is this output).
usage: gpu_summary_probe.py [--reps 5] [--parent DIR] [--workloads grid,config3,single] [--no-route]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as g

HBM_BYTES_PER_MS = 8e9  # 8 TB/s
LEVELS = (500, 950, 990)


def load_other(root):
    """The package of another checkout (its own library), under a module name of its own."""
    d = os.path.join(root, "5g-nr-randomaccess_amd")
    spec = importlib.util.spec_from_file_location("nr_randomaccess_amd_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workloads", default="grid,config3,single")
    ap.add_argument("--no-route", action="store_true", help="skip (c)")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    other = load_other(args.parent) if args.parent else pkg
    oeng = other.Engine(0) if args.parent else eng
    grid = lambda p, v: [p.make_cfg(n, variant=v, rng_mode=p.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda p: grid(p, p.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda p: grid(p, p.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda p: [p.make_cfg(100000, variant=p.VARIANT_BETA_C, rng_mode=p.RNG_PHILOX, seed=0)])}
    med = statistics.median
    print(f"timeline and sojourn calls of: {'--parent ' + args.parent if args.parent else 'this checkout'}; reps {args.reps}\n")
    print("| workload | (a) timeline total_ms (spread) | timeline_ms | threads | (b) summary total_ms (spread) | summary_ms (spread) | (b) / (a) | summary_ms / timeline_ms | byte floor (ms) | "
          "summary_ms / floor | (c) sojourn route (ms) | (c) / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, ocfgs = make(pkg), make(other)
        groups = [k % 10 for k in range(len(cfgs))] if len(cfgs) > 1 else None
        ngroups = 10 if groups else 1
        oeng.run_trials_timeline(ocfgs, 2002, 5, groups=groups, ngroups=ngroups)  # warm-up: the arena, the code objects
        rows = {}
        for threads in (512, 1024):
            eng.set("summary_threads", threads)
            eng.run_trials_summary(cfgs, LEVELS)
            a_tot, a_ms, tot, sms = [], [], [], []
            for _ in range(args.reps):  # (a) and (b) alternate
                oeng.run_trials_timeline(ocfgs, 2002, 5, groups=groups, ngroups=ngroups)
                tm = oeng.timing()
                a_tot.append(tm.total_ms); a_ms.append(tm.timeline_ms)
                res, _, sm = eng.run_trials_summary(cfgs, LEVELS)
                tm = eng.timing()
                tot.append(tm.total_ms); sms.append(tm.summary_ms)
            rows[threads] = (a_tot, a_ms, tot, sms, sm)
        assert rows[512][4].rows.tobytes() == rows[1024][4].rows.tobytes(), "the two workgroup shapes disagree"
        sm = rows[1024][4]
        assert not sm.rows["status"].any() and not sm.rows["range_errors"].any()
        floor = 2 * 48 * sum(c.nUE for c in cfgs) / HBM_BYTES_PER_MS
        c_ms = [float("nan")]
        if len(cfgs) > 1 and not args.no_route:
            c_ms = []
            for _ in range(max(1, args.reps // 2)):
                t0 = time.perf_counter()
                _, _, sj = oeng.run_trials_sojourn(ocfgs, 1, 70000, 10012, 1)  # one group per trial, one row
                q = [[sj.quantile(k, -1, m / 1000.0) for m in LEVELS] for k in range(len(ocfgs))]
                c_ms.append(1e3 * (time.perf_counter() - t0))
            assert [r[0] for r in q] == sm.rows["q"][:, 0, 0].tolist(), "the two routes disagree on the median"
        sp = lambda v: f"{med(v):.2f} ({max(v) - min(v):.2f})"
        for threads in (512, 1024):
            a_tot, a_ms, tot, sms, _ = rows[threads]
            print(f"| {name} | {sp(a_tot)} | {med(a_ms):.3f} | {threads} | {sp(tot)} | {med(sms):.3f} ({max(sms) - min(sms):.3f}) | {med(tot) / med(a_tot):.3f} | "
                  f"{med(sms) / med(a_ms):.2f} | {floor:.4f} | {med(sms) / floor:.1f} | {med(c_ms):.0f} | {med(c_ms) / med(tot):.1f} |", flush=True)
    eng.close()
    if args.parent:
        oeng.close()


if __name__ == "__main__":
    main()
