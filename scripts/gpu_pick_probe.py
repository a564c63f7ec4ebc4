"""What a pick costs (prach_run_trials_pick, csrc/prach_pick.hip), on the three workloads of DESIGN.md 4: the 1000-trial Beta.c grid, BASELINE config 3 (the
same grid of RandomAccessWithNOMA) and one 100 000-UE trial; the spec is LARGEST sojourn, k = 16, over the served.  Per workload, in ONE run, medians of
repeated calls after a warm-up call:
  (a) total_ms and summary_ms of prach_run_trials_summary (levels 500, 950, 990) on the same inputs: the summary kernel has the same launch shape (one
      workgroup per trial) and reads the same records in two passes of 48 B per UE, the pick kernel in three of 32 B here.  With --parent DIR the summary
      call is the one of the library built in that checkout (another commit), loaded next to this one; calls (a), (b) and (d) alternate
  (b) total_ms and pick_ms of prach_run_trials_pick without host logs, per workgroup shape (engine option pick_threads), the spread (max - min over the
      repetitions) beside the median
  (c) the only route of a library without the pick to the same rows: prach_run_trials with EVERY per-UE log (--parent's, where given) plus the filter and
      sort on the host (this checkout's prach_pick_from_logs) — wall time, host part included.  The probe asserts that its headers and rows equal (b)'s
  (d) kernel_ms of plain prach_run_trials of both libraries: no simulation kernel differs between them
and, beside pick_ms, the kernel's byte floor: 3 passes x 32 B of the 64-byte record per UE (two 16-byte loads), over 8 TB/s.  Prints one markdown table
(profiles/pick_kernel.md is this output).
usage: gpu_pick_probe.py [--reps 5] [--parent DIR] [--workloads grid,config3,single] [--no-route]"""
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
SPEC = ((), "largest", "sojourn", 16, 1)  # where, order, key, k, who = served


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
    print(f"summary, log and plain calls (a), (c), (d) of: {'--parent ' + args.parent if args.parent else 'this checkout'}; reps {args.reps}\n")
    print("| workload | (a) summary total_ms (spread) | summary_ms | threads | (b) pick total_ms (spread) | pick_ms (spread) | (b) / (a) | pick_ms / summary_ms | byte floor (ms) | "
          "pick_ms / floor | (c) logs + host filter (ms) | (c) / (b) | (d) kernel_ms there (spread) | (d) kernel_ms here (spread) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, ocfgs = make(pkg), make(other)
        oeng.run_trials_summary(ocfgs, LEVELS)  # warm-up: the arena, the code objects
        oeng.run_trials(ocfgs)
        eng.run_trials(cfgs)
        rows = {}
        for threads in (512, 1024):
            eng.set("pick_threads", threads)
            eng.run_trials_pick(cfgs, *SPEC)
            a_tot, a_ms, tot, pms, d_there, d_here = [], [], [], [], [], []
            for _ in range(args.reps):  # (a), (b) and (d) alternate
                oeng.run_trials_summary(ocfgs, LEVELS)
                tm = oeng.timing()
                a_tot.append(tm.total_ms); a_ms.append(tm.summary_ms)
                res, _, pk = eng.run_trials_pick(cfgs, *SPEC)
                tm = eng.timing()
                tot.append(tm.total_ms); pms.append(tm.pick_ms)
                oeng.run_trials(ocfgs)
                d_there.append(oeng.timing().kernel_ms)
                eng.run_trials(cfgs)
                d_here.append(eng.timing().kernel_ms)
            rows[threads] = (a_tot, a_ms, tot, pms, d_there, d_here, pk, res)
        assert rows[512][6].same_as(rows[1024][6]), "the two workgroup shapes disagree"
        pk, res = rows[1024][6], rows[1024][7]
        assert not pk.headers["status"].any() and not pk.headers["range_errors"].any()
        floor = 3 * 32 * sum(c.nUE for c in cfgs) / HBM_BYTES_PER_MS
        c_ms = [float("nan")]
        if not args.no_route:
            c_ms = []
            for _ in range(max(1, args.reps // 2)):
                t0 = time.perf_counter()
                ores, logs = oeng.run_trials(ocfgs, want_logs=True)
                host = pkg.pick_from_logs(cfgs, [r.steps for r in ores], logs, *SPEC)
                c_ms.append(1e3 * (time.perf_counter() - t0))
                del logs
            assert host.same_as(pk), "the two routes disagree"
        sp = lambda v: f"{med(v):.2f} ({max(v) - min(v):.2f})"
        for threads in (512, 1024):
            a_tot, a_ms, tot, pms, d_there, d_here, _, _ = rows[threads]
            print(f"| {name} | {sp(a_tot)} | {med(a_ms):.3f} | {threads} | {sp(tot)} | {med(pms):.3f} ({max(pms) - min(pms):.3f}) | {med(tot) / med(a_tot):.3f} | "
                  f"{med(pms) / med(a_ms):.2f} | {floor:.4f} | {med(pms) / floor:.1f} | {med(c_ms):.0f} | {med(c_ms) / med(tot):.1f} | {sp(d_there)} | {sp(d_here)} |", flush=True)
    eng.close()
    if args.parent:
        oeng.close()


if __name__ == "__main__":
    main()
