"""What the distributions cost (prach_run_trials_dist, csrc/prach_dist.hip), on three workloads: the 1000-trial Beta.c grid, BASELINE config 3 (the
same grid of RandomAccessWithNOMA) and one 100 000-UE trial.  Per workload, in ONE run, medians of repeated calls after a warm-up call:
  (a) total_ms of prach_run_trials without logs (the call as it was before the distributions existed)
  (b) total_ms and dist_ms of prach_run_trials_dist without logs, for every binning scheme of the preamble counts (engine option dist_scheme)
  (c) the only other way to the same histograms: the same trials with the per-UE logs of every trial + np.bincount on the host, in slices
      of --slice trials (the logs of a whole grid are 3.5 GB), the slices' times summed
and, beside dist_ms, the kernel's own bytes over 8 TB/s: 4 B of timers per UE, 4 B of preamble counts (int32 form) or the 32-byte sector of a
successful UE's record (batch kernel), 8 B per flushed bin.  Prints one markdown table (profiles/dist_kernel.md is this output).
usage: gpu_dist_probe.py [--reps 5] [--slice 100] [--bins 4096] [--workloads grid,config3,single]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import __graft_entry__ as g

HBM_BYTES_PER_MS = 8e9  # 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice", type=int, default=100)
    ap.add_argument("--bins", type=int, default=4096)
    ap.add_argument("--workloads", default="grid,config3,single")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    grid = lambda v: [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda: grid(pkg.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda: grid(pkg.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda: [pkg.make_cfg(100000, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=0)])}
    med = statistics.median
    print("| workload | (a) run_trials total_ms | scheme | (b) run_trials_dist total_ms | dist_ms | launches | kernel bytes / 8 TB/s (ms) | (c) logs + np.bincount (ms) | (c) / (b) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs = make()
        groups = [k % 10 for k in range(len(cfgs))] if len(cfgs) > 1 else None
        ngroups = 10 if groups else 1
        eng.run_trials(cfgs)  # warm-up: the arena, the code objects
        a = []
        for _ in range(args.reps):
            eng.run_trials(cfgs)
            a.append(eng.timing().total_ms)
        b = {}
        for scheme in (0, 1, 2):
            eng.set("dist_scheme", scheme)
            eng.run_trials_dist(cfgs, args.bins, 1, groups=groups, ngroups=ngroups)
            tot, dms = [], []
            for _ in range(args.reps):
                res, _, d = eng.run_trials_dist(cfgs, args.bins, 1, groups=groups, ngroups=ngroups)
                tm = eng.timing()
                tot.append(tm.total_ms); dms.append(tm.dist_ms)
            b[scheme] = (med(tot), med(dms), tm.launches, tm.rec_mode)
        eng.set("dist_scheme", 1)
        ues, succ = sum(c.nUE for c in cfgs), int(d.success.sum())
        tiles = sum(-(-c.nUE // pkg.dist_tile_ues()) for c in cfgs)
        flushed = tiles * (int(np.count_nonzero(d.delay_hist)) // ngroups + int(np.count_nonzero(d.ptc_hist)) // ngroups)  # upper bound: every tile flushes its group's non-empty bins
        own = 4 * ues + (32 * succ if b[1][3] == 4 else 4 * ues) + 8 * flushed
        # (c) per-UE logs of every trial over the bus + the histogram on the host, in slices
        c_ms = []
        for rep in range(max(1, args.reps // 2)):
            t0 = time.perf_counter()
            ref = pkg.Dist(ngroups, args.bins, 1)
            for lo in range(0, len(cfgs), args.slice):
                part = cfgs[lo:lo + args.slice]
                _, logs = eng.run_trials(part, want_logs=True)
                for k, lg in enumerate(logs):
                    u = np.frombuffer(lg, dtype=np.int32).reshape(-1, 16)
                    ok = u[:, 14] == 1
                    gq = (lo + k) % 10 if groups else 0
                    ref.delay_hist[gq] += np.bincount(np.minimum(u[ok, 1], args.bins), minlength=args.bins + 1)[:args.bins].astype(np.uint64)
                    ref.ptc_hist[gq] += np.bincount(np.minimum(u[ok, 11], 255), minlength=256).astype(np.uint64)
            c_ms.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(ref.delay_hist, d.delay_hist) and np.array_equal(ref.ptc_hist, d.ptc_hist), "the two ways disagree"
        for scheme in (0, 1, 2):
            tot, dms, launches, _ = b[scheme]
            print(f"| {name} | {med(a):.2f} | {scheme} | {tot:.2f} | {dms:.3f} | {launches} | {own / HBM_BYTES_PER_MS:.4f} | {med(c_ms):.0f} | {med(c_ms) / tot:.1f} |", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
