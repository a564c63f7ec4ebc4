"""What the per-UE columns cost (prach_run_trials_columns, csrc/prach_columns.hip), on the three workloads of DESIGN.md 4: the 1000-trial Beta.c grid,
BASELINE config 3 (the same grid of RandomAccessWithNOMA) and one 100 000-UE trial.  Two field sets: (arrival, sojourn, state) and all 16 raw words.  Per
workload, in ONE run, medians of repeated calls after a warm-up call, the spread (max - min over the repetitions) beside the median:
  (a) xtab_ms of prach_run_trials_xtab (the default table) on the same inputs: the cross-tabulation has the same tile shape and reads the same records.
      With --parent DIR the call is the one of the library built in that checkout (another commit), loaded next to this one; (a), (b) and (e) alternate
  (b) total_ms and columns_ms of the call with the HOST destination, per field set, and the kernel's byte floor beside columns_ms: 48 B (32 B + the quarter
      with nowBackoff) or 64 B read plus 4 B per column written, per UE, over 8 TB/s
  (c) wall time of the call with the DEVICE destination (a torch tensor; torch is imported first, so that the process has one HIP runtime)
  (d) the only route of a library without the columns to the same arrays: prach_run_trials with EVERY per-UE log (--parent's, where given) plus the
      derivation in numpy — wall time, host part included.  The probe asserts that its arrays equal (b)'s
  (e) kernel_ms of plain prach_run_trials of both libraries: no simulation kernel differs between them
Prints one markdown table (profiles/columns_kernel.md is this output).
usage: gpu_columns_probe.py [--reps 5] [--parent DIR] [--workloads grid,config3,single] [--no-route]"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import torch  # noqa: F401  (before the package loads its library: Engine.run_trials_columns(device=True))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as g  # noqa: E402

HBM_BYTES_PER_MS = 8e9  # 8 TB/s
SETS = {"arrival,sojourn,state": (["arrival", "sojourn", "state"], 48), "16 raw words": (["raw:" + n for n in g.load_package().UE_FIELDS], 64)}


def load_other(root):
    """The package of another checkout (its own library), under a module name of its own."""
    d = os.path.join(root, "5g-nr-randomaccess_amd")
    spec = importlib.util.spec_from_file_location("nr_randomaccess_amd_parent", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def numpy_route(pkg, cfgs, logs):
    """(arrival, sojourn, state) of every UE from the 64-byte records, restated on the host: a(i), the classes and the STATE rule of include/prach.h."""
    out = np.empty((3, sum(c.nUE for c in cfgs)), dtype=np.int32)
    o = 0
    scheds = {}
    for c, lg in zip(cfgs, logs):
        a = np.frombuffer(lg, dtype=np.int32).reshape(-1, 16)
        key = (c.nUE, c.uniform, c.accessTime, c.variant)
        if key not in scheds:
            scheds[key] = c.accessTime * np.searchsorted(np.asarray(pkg.arrival_schedule(c)[0], dtype=np.int64), np.arange(c.nUE), side="right")
        at, idle = scheds[key], a[:, 2] == -1
        served = ~idle & (a[:, 14] == 1)
        un = np.where(a[:, 2] == 1, np.where(a[:, 6] > 0, 2, 3), np.where(a[:, 2] == 2, np.where(a[:, 13] < 48, 4, 5), 6))
        seg = out[:, o:o + c.nUE]
        seg[0] = np.where(idle, -1, at)
        seg[1] = np.where(served, a[:, 3].astype(np.int64) + 6 - at, -1)
        seg[2] = np.where(idle, 0, np.where(served, 1, un))
        o += c.nUE
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workloads", default="grid,config3,single")
    ap.add_argument("--no-route", action="store_true", help="skip (d)")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    other = load_other(args.parent) if args.parent else pkg
    oeng = other.Engine(0) if args.parent else eng
    grid = lambda p, v: [p.make_cfg(n, variant=v, rng_mode=p.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda p: grid(p, p.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda p: grid(p, p.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda p: [p.make_cfg(100000, variant=p.VARIANT_BETA_C, rng_mode=p.RNG_PHILOX, seed=0)])}
    med = statistics.median
    sp = lambda v, d=2: f"{med(v):.{d}f} ({max(v) - min(v):.{d}f})"
    print(f"xtab, log and plain calls (a), (d), (e) of: {'--parent ' + args.parent if args.parent else 'this checkout'}; reps {args.reps}\n")
    print("| workload | fields | (a) xtab_ms (spread) | (b) host: total_ms (spread) | columns_ms (spread) | byte floor (ms) | columns_ms / floor | columns_ms / xtab_ms | "
          "(c) device: wall ms (spread) | (d) logs + numpy (ms) | (d) / (b) | (d) / (c) | (e) kernel_ms there (spread) | (e) kernel_ms here (spread) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, ocfgs = make(pkg), make(other)
        nue = sum(c.nUE for c in cfgs)
        oeng.run_trials_xtab(ocfgs)  # warm-up: the arena, the code objects
        oeng.run_trials(ocfgs)
        eng.run_trials(cfgs)
        d_ms, route = [float("nan")], None
        if not args.no_route:
            d_ms = []
            for _ in range(max(1, args.reps // 2)):
                t0 = time.perf_counter()
                ores, logs = oeng.run_trials(ocfgs, want_logs=True)
                route = numpy_route(pkg, cfgs, logs)
                d_ms.append(1e3 * (time.perf_counter() - t0))
                del logs
        for label, (fields, read_bytes) in SETS.items():
            eng.run_trials_columns(cfgs, fields)
            eng.run_trials_columns(cfgs, fields, device=True)
            x_ms, tot, cms, dev, e_there, e_here = [], [], [], [], [], []
            for _ in range(args.reps):  # (a), (b), (c) and (e) alternate
                oeng.run_trials_xtab(ocfgs)
                x_ms.append(oeng.timing().xtab_ms)
                res, _, col = eng.run_trials_columns(cfgs, fields)
                tm = eng.timing()
                tot.append(tm.total_ms); cms.append(tm.columns_ms)
                t0 = time.perf_counter()
                _, _, dcol = eng.run_trials_columns(cfgs, fields, device=True)
                dev.append(1e3 * (time.perf_counter() - t0))
                oeng.run_trials(ocfgs)
                e_there.append(oeng.timing().kernel_ms)
                eng.run_trials(cfgs)
                e_here.append(eng.timing().kernel_ms)
            assert not col.headers["status"].any() and bool((dcol.data.cpu() == torch.from_numpy(col.data)).all()), "the two destinations disagree"
            if route is not None and len(fields) == 3:
                assert np.array_equal(route, col.data), "the two routes disagree"
            del col, dcol
            floor = (read_bytes + 4 * len(fields)) * nue / HBM_BYTES_PER_MS
            dd = med(d_ms) if len(fields) == 3 else float("nan")  # (the numpy route derives the three fields)
            print(f"| {name} | {label} | {sp(x_ms, 3)} | {sp(tot)} | {sp(cms, 3)} | {floor:.4f} | {med(cms) / floor:.1f} | {med(cms) / med(x_ms):.2f} | {sp(dev)} | {dd:.0f} | "
                  f"{dd / med(tot):.1f} | {dd / med(dev):.1f} | {sp(e_there)} | {sp(e_here)} |", flush=True)
    eng.close()
    if args.parent:
        oeng.close()


if __name__ == "__main__":
    main()
