"""What the timelines cost (prach_run_trials_timeline, csrc/prach_timeline.hip), on three workloads: the 1000-trial Beta.c grid, BASELINE config 3 (the
same grid of RandomAccessWithNOMA) and one 100 000-UE trial; bins of 5 ms over the horizon, ten groups.  Per workload, in ONE run, medians of repeated
calls after a warm-up call:
  (a) total_ms of prach_run_trials without logs
  (b) total_ms and timeline_ms of prach_run_trials_timeline without host logs, under both binning schemes (engine option timeline_scheme)
  (c) the only other way to the same timelines: the same trials with the per-UE logs of every trial + the numpy restatement on the host, in slices
      of --slice trials (the logs of a whole grid are 3.5 GB), the slices' times summed; the probe asserts that (b) and (c) agree
and, beside timeline_ms, the kernel's byte floor: 64 B per UE plus 8 B per flushed bin, over 8 TB/s.  (b) - (a) is what writing the device logs and
reducing them costs.  Prints one markdown table (profiles/timeline_kernel.md is this output).
usage: gpu_timeline_probe.py [--reps 5] [--slice 100] [--bin-ms 5] [--workloads grid,config3,single]"""
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
TIMER, ACTIVE, TXTIME, FLAG = 1, 2, 3, 14


def numpy_add(tl, gq, u, sched, access_time):
    """The numpy restatement of prach_timeline_accumulate_logs for one trial (int32 [nUE, 16]) into group gq."""
    bins, w = tl.bins, tl.bin_ms
    at = access_time * np.searchsorted(sched, np.arange(len(u)), side="right")
    arrived, ok = u[:, ACTIVE] != -1, u[:, FLAG] == 1
    c, timer = u[:, TXTIME].astype(np.int64) + 6, u[:, TIMER].astype(np.int64)
    ab, db = at // w, c // w
    inb = ok & (ab < bins)
    tl.series["arrivals"][gq] += np.bincount(ab[arrived & (ab < bins)], minlength=bins).astype(np.uint64)
    tl.series["success"][gq] += np.bincount(ab[inb], minlength=bins).astype(np.uint64)
    tl.series["sojourn_sum"][gq] += np.bincount(ab[inb], weights=(c - at)[inb], minlength=bins).astype(np.uint64)
    tl.series["timer_sum"][gq] += np.bincount(ab[inb], weights=timer[inb], minlength=bins).astype(np.uint64)
    tl.series["done"][gq] += np.bincount(db[ok & (db < bins)], minlength=bins).astype(np.uint64)
    tl.scalars["restarted"][gq] += int((ok & (c - timer != at)).sum())
    tl.scalars["sojourn_sum"][gq] += int((c - at)[ok].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice", type=int, default=100)
    ap.add_argument("--bin-ms", type=int, default=5)
    ap.add_argument("--workloads", default="grid,config3,single")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    w = args.bin_ms
    bins = -(-(10000 + 6) // w)
    grid = lambda v: [pkg.make_cfg(n, variant=v, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda: grid(pkg.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda: grid(pkg.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda: [pkg.make_cfg(100000, variant=pkg.VARIANT_BETA_C, rng_mode=pkg.RNG_PHILOX, seed=0)])}
    med = statistics.median
    print("| workload | (a) run_trials total_ms | scheme | (b) run_trials_timeline total_ms | timeline_ms | (b) - (a) | launches | byte floor (ms) | (c) logs + numpy (ms) | (c) / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
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
        for scheme in (0, 1):
            eng.set("timeline_scheme", scheme)
            eng.run_trials_timeline(cfgs, bins, w, groups=groups, ngroups=ngroups)  # warm-up: the arena grows by the device logs
            tot, tms = [], []
            for _ in range(args.reps):
                _, _, tl = eng.run_trials_timeline(cfgs, bins, w, groups=groups, ngroups=ngroups)
                tm = eng.timing()
                tot.append(tm.total_ms); tms.append(tm.timeline_ms)
            b[scheme] = (med(tot), med(tms), tm.launches, tl)
        eng.set("timeline_scheme", 1)
        assert b[0][3].same_as(b[1][3]), "the two schemes disagree"
        tl = b[1][3]
        ues = sum(c.nUE for c in cfgs)
        tiles = sum(-(-c.nUE // pkg.timeline_tile_ues()) for c in cfgs)
        flushed = tiles * sum(int(np.count_nonzero(tl.series[n])) for n in pkg.TIMELINE_SERIES) // ngroups  # upper bound: every tile flushes its group's non-zero bins
        floor = (64 * ues + 8 * min(flushed, 5 * ues)) / HBM_BYTES_PER_MS
        # (c) per-UE logs of every trial over the bus + the numpy restatement on the host, in slices
        c_ms = []
        scheds = {}
        for rep in range(max(1, args.reps // 2)):
            t0 = time.perf_counter()
            ref = pkg.Timeline(ngroups, bins, w)
            for lo in range(0, len(cfgs), args.slice):
                part = cfgs[lo:lo + args.slice]
                _, logs = eng.run_trials(part, want_logs=True)
                for k, lg in enumerate(logs):
                    c = part[k]
                    if (c.nUE, c.accessTime) not in scheds:
                        scheds[(c.nUE, c.accessTime)] = np.asarray(pkg.arrival_schedule(c)[0], dtype=np.int64)
                    numpy_add(ref, (lo + k) % 10 if groups else 0, np.frombuffer(lg, dtype=np.int32).reshape(-1, 16), scheds[(c.nUE, c.accessTime)], c.accessTime)
            c_ms.append(1e3 * (time.perf_counter() - t0))
        assert all(np.array_equal(ref.series[n], tl.series[n]) for n in pkg.TIMELINE_SERIES), "the two ways disagree"
        assert np.array_equal(ref.scalars["restarted"], tl.scalars["restarted"]) and np.array_equal(ref.scalars["sojourn_sum"], tl.scalars["sojourn_sum"])
        for scheme in (0, 1):
            tot, tms, launches, _ = b[scheme]
            print(f"| {name} | {med(a):.2f} | {scheme} | {tot:.2f} | {tms:.3f} | {tot - med(a):.2f} | {launches} | {floor:.4f} | {med(c_ms):.0f} | {med(c_ms) / tot:.1f} |", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
