"""What the sojourn histograms cost (prach_run_trials_sojourn, csrc/prach_sojourn.hip), on the three workloads of DESIGN.md 4: the 1000-trial Beta.c
grid, BASELINE config 3 (the same grid of RandomAccessWithNOMA) and one 100 000-UE trial; rows of 500 ms, delay bins of 5 ms over the horizon, ten
groups.  Per workload, in ONE run, medians of repeated calls after a warm-up call:
  (a) total_ms and timeline_ms of prach_run_trials_timeline (5 ms bins) on the same inputs: both calls lay out every trial's log on the device, so the
      byte floor of 64 B per UE is the same.  With --parent DIR the timeline call is the one of the library built in that checkout (another commit),
      loaded next to this one; calls (a) and (b) alternate
  (b) total_ms and sojourn_ms of prach_run_trials_sojourn without host logs, under both binning schemes (engine option sojourn_scheme), the spread
      (max - min over the repetitions) beside the median
  (c) the only other way to the same histograms: the same trials with the per-UE logs of every trial + numpy on the host, in slices of --slice trials,
      the slices' times summed; the probe asserts that (b) and (c) agree
and, beside sojourn_ms, the kernel's byte floor: 64 B per UE plus 8 B per flushed counter, over 8 TB/s.  Prints one markdown table
(profiles/sojourn_kernel.md is this output).
usage: gpu_sojourn_probe.py [--reps 5] [--slice 100] [--parent DIR] [--workloads grid,config3,single] [--no-host]"""
import argparse
import importlib.util
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


def numpy_add(sj, gq, u, sched, access_time):
    """numpy restatement of prach_sojourn_accumulate_logs for one trial (int32 [nUE, 16]) into group gq: one flattened bincount."""
    rows, rw, bins, bw = sj.arrival_bins, sj.arrival_bin_ms, sj.delay_bins, sj.delay_bin_ms
    at = access_time * np.searchsorted(sched, np.arange(len(u)), side="right")
    arrived, ok = u[:, ACTIVE] != -1, u[:, FLAG] == 1
    soj = u[:, TXTIME].astype(np.int64) + 6 - at
    r, d = at // rw, soj // bw
    cell = ok & (r < rows) & (d < bins)
    sj.hist[gq] += np.bincount(r[cell] * bins + d[cell], minlength=rows * bins).reshape(rows, bins).astype(np.uint64)
    sj.row_arrived[gq] += np.bincount(r[arrived & (r < rows)], minlength=rows).astype(np.uint64)
    sj.row_delay_overflow[gq] += np.bincount(r[ok & (r < rows) & (d >= bins)], minlength=rows).astype(np.uint64)
    sj.scalars["sojourn_sum"][gq] += int(soj[ok].sum())


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
    ap.add_argument("--slice", type=int, default=100)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--workloads", default="grid,config3,single")
    ap.add_argument("--no-host", action="store_true", help="skip (c)")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    other = load_other(args.parent) if args.parent else pkg
    oeng = other.Engine(0) if args.parent else eng
    spec = (20, 500, 2002, 5)
    tl_bins = 2002
    grid = lambda p, v: [p.make_cfg(n, variant=v, rng_mode=p.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda p: grid(p, p.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda p: grid(p, p.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda p: [p.make_cfg(100000, variant=p.VARIANT_BETA_C, rng_mode=p.RNG_PHILOX, seed=0)])}
    med = statistics.median
    print(f"timeline call of: {'--parent ' + args.parent if args.parent else 'this checkout'}; reps {args.reps}\n")
    print("| workload | (a) timeline total_ms (spread) | timeline_ms | scheme | (b) sojourn total_ms (spread) | sojourn_ms (spread) | (b) / (a) | byte floor (ms) | sojourn_ms / floor | (c) logs + numpy (ms) | (c) / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, ocfgs = make(pkg), make(other)
        groups = [k % 10 for k in range(len(cfgs))] if len(cfgs) > 1 else None
        ngroups = 10 if groups else 1
        oeng.run_trials_timeline(ocfgs, tl_bins, 5, groups=groups, ngroups=ngroups)  # warm-up: the arena, the code objects
        rows = {}
        for scheme in (0, 1):
            eng.set("sojourn_scheme", scheme)
            eng.run_trials_sojourn(cfgs, *spec, groups=groups, ngroups=ngroups)
            a_tot, a_ms, tot, sms = [], [], [], []
            for _ in range(args.reps):  # (a) and (b) alternate
                oeng.run_trials_timeline(ocfgs, tl_bins, 5, groups=groups, ngroups=ngroups)
                tm = oeng.timing()
                a_tot.append(tm.total_ms); a_ms.append(tm.timeline_ms)
                _, _, sj = eng.run_trials_sojourn(cfgs, *spec, groups=groups, ngroups=ngroups)
                tm = eng.timing()
                tot.append(tm.total_ms); sms.append(tm.sojourn_ms)
            rows[scheme] = (a_tot, a_ms, tot, sms, sj)
        assert rows[0][4].same_as(rows[1][4]), "the two schemes disagree"
        sj = rows[1][4]
        ues = sum(c.nUE for c in cfgs)
        tiles = sum(-(-c.nUE // pkg.sojourn_tile_ues()) for c in cfgs)
        flushed = tiles * sum(int(np.count_nonzero(a)) for a in sj._arrays()) // ngroups  # upper bound: every tile flushes its group's non-zero counters
        floor = (64 * ues + 8 * min(flushed, 3 * ues)) / HBM_BYTES_PER_MS
        c_ms, scheds = [], {}
        for rep in range(0 if args.no_host else max(1, args.reps // 2)):
            t0 = time.perf_counter()
            ref = pkg.Sojourn(ngroups, *spec)
            for lo in range(0, len(cfgs), args.slice):
                part = cfgs[lo:lo + args.slice]
                _, logs = eng.run_trials(part, want_logs=True)
                for k, lg in enumerate(logs):
                    c = part[k]
                    if (c.nUE, c.accessTime) not in scheds:
                        scheds[(c.nUE, c.accessTime)] = np.asarray(pkg.arrival_schedule(c)[0], dtype=np.int64)
                    numpy_add(ref, (lo + k) % 10 if groups else 0, np.frombuffer(lg, dtype=np.int32).reshape(-1, 16), scheds[(c.nUE, c.accessTime)], c.accessTime)
            c_ms.append(1e3 * (time.perf_counter() - t0))
        if c_ms:
            assert all(np.array_equal(x, y) for x, y in zip(ref._arrays(), sj._arrays())), "the two ways disagree"
            assert np.array_equal(ref.scalars["sojourn_sum"], sj.scalars["sojourn_sum"])
        else:
            c_ms = [float("nan")]
        sp = lambda v: f"{med(v):.2f} ({max(v) - min(v):.2f})"
        for scheme in (0, 1):
            a_tot, a_ms, tot, sms, _ = rows[scheme]
            print(f"| {name} | {sp(a_tot)} | {med(a_ms):.3f} | {scheme} | {sp(tot)} | {med(sms):.3f} ({max(sms) - min(sms):.3f}) | {med(tot) / med(a_tot):.3f} | {floor:.4f} | "
                  f"{med(sms) / floor:.1f} | {med(c_ms):.0f} | {med(c_ms) / med(tot):.1f} |", flush=True)
    eng.close()
    if args.parent:
        oeng.close()


if __name__ == "__main__":
    main()
