"""What the outcome cross-tabulation costs (prach_run_trials_xtab, csrc/prach_xtab.hip), on the three workloads of DESIGN.md 4: the 1000-trial Beta.c grid,
BASELINE config 3 (the same grid of RandomAccessWithNOMA) and one 100 000-UE trial; ten groups on the grids.  Two specs: the drivers' default
(arrival:500:20 x state:1:7, everybody) and (arrival:500:20 x age:5:2002, the unserved).  Per workload, in ONE run, medians of repeated calls after a warm-up:
  (p) the run-to-run spread of the sojourn call (20 x 500 ms rows, 2002 x 5 ms bins) of the library of --parent DIR (another commit, loaded next to this
      one; without --parent: this checkout's), measured first, on its own
  (a) total_ms and sojourn_ms of that call, alternating with
  (b) total_ms and xtab_ms of prach_run_trials_xtab without host logs, per spec and scheme (engine option xtab_scheme)
  (c) the only other way to the same tables: the per-UE logs of every trial + numpy on the host, in slices of --slice trials; the probe asserts that (b)
      and (c) agree
  (d) with --onecopy DIR, xtab_ms of the library built there with -DPRACH_XT_COPY_WORDS=0 (plain LDS adds into ONE copy of the table) against this
      checkout's per-wavefront copies, alternating, default spec, scheme 1
and, beside xtab_ms, the kernel's byte floor: the words of a record the spec makes a lane read (32 B, + 16 B with STATE, + 16 B with PTC) per UE over
8 TB/s, and the UEs that reached a cell (under scheme 0, and in a table past the LDS window, one global atomic each).  Prints markdown tables (profiles/xtab_kernel.md holds this output).
usage: gpu_xtab_probe.py [--reps 5] [--slice 100] [--parent DIR] [--onecopy DIR] [--workloads grid,config3,single] [--specs default,ages] [--no-host]"""
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
TIMER, ACTIVE, TXTIME, NOWBACKOFF, CONNREQ, FLAG = 1, 2, 3, 6, 13, 14


def numpy_table(spec, u, sched, access_time, E):
    """numpy restatement of the two probe specs for one trial (int32 [nUE, 16]): the cells of one group."""
    (_, rw, rb), (cf, cw, cb), who = spec
    at = access_time * np.searchsorted(sched, np.arange(len(u)), side="right")
    idle = u[:, ACTIVE] == -1
    served = ~idle & (u[:, FLAG] == 1)
    if cf == "state":
        un = np.where(u[:, ACTIVE] == 1, np.where(u[:, NOWBACKOFF] > 0, 2, 3), np.where(u[:, ACTIVE] == 2, np.where(u[:, CONNREQ] < 48, 4, 5), 6))
        cv = np.where(idle, 0, np.where(served, 1, un))
    else:
        cv = E - at
    sel = (np.where(idle, 4, np.where(served, 1, 2)) & who) != 0
    good = sel & ~idle & (cv >= 0)
    r, c = np.minimum(at[good] // rw, rb), np.minimum(cv[good] // cw, cb)
    return np.bincount(r * (cb + 1) + c, minlength=(rb + 1) * (cb + 1)).reshape(rb + 1, cb + 1).astype(np.uint64)


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
    ap.add_argument("--slice", type=int, default=100)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--onecopy", default=None)
    ap.add_argument("--workloads", default="grid,config3,single")
    ap.add_argument("--specs", default="default,ages")
    ap.add_argument("--no-host", action="store_true", help="skip (c)")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    other = load_other(args.parent, "nr_randomaccess_amd_parent") if args.parent else pkg
    oeng = other.Engine(0) if args.parent else eng
    one = load_other(args.onecopy, "nr_randomaccess_amd_onecopy") if args.onecopy else None
    one_eng = one.Engine(0) if one else None
    sj_spec = (20, 500, 2002, 5)
    specs = {"default": (("arrival", 500, 20), ("state", 1, 7), 7), "ages": (("arrival", 500, 20), ("age", 5, 2002), 2)}
    bytes_per_ue = {"default": 48, "ages": 32}
    grid = lambda p, v: [p.make_cfg(n, variant=v, rng_mode=p.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda p: grid(p, p.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda p: grid(p, p.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda p: [p.make_cfg(100000, variant=p.VARIANT_BETA_C, rng_mode=p.RNG_PHILOX, seed=0)])}
    med = statistics.median
    sp = lambda v, d=2: f"{med(v):.{d}f} ({max(v) - min(v):.{d}f})"
    print(f"sojourn call of: {'--parent ' + args.parent if args.parent else 'this checkout'}; reps {args.reps}\n")
    main_rows, copy_rows, spread_rows = [], [], []
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, ocfgs = make(pkg), make(other)
        groups = [k % 10 for k in range(len(cfgs))] if len(cfgs) > 1 else None
        ngroups = 10 if groups else 1
        ues = sum(c.nUE for c in cfgs)
        oeng.run_trials_sojourn(ocfgs, *sj_spec, groups=groups, ngroups=ngroups)  # warm-up: the arena, the code objects
        p_tot, p_ms = [], []
        for _ in range(args.reps):  # (p) the parent's own spread, before anything else
            oeng.run_trials_sojourn(ocfgs, *sj_spec, groups=groups, ngroups=ngroups)
            tm = oeng.timing()
            p_tot.append(tm.total_ms); p_ms.append(tm.sojourn_ms)
        spread_rows.append(f"| {name} | {sp(p_tot)} | {sp(p_ms, 3)} |")
        for sname in args.specs.split(","):
            spec = specs[sname]
            got = {}
            for scheme in (0, 1):
                eng.set("xtab_scheme", scheme)
                eng.run_trials_xtab(cfgs, *spec, groups=groups, ngroups=ngroups)
                a_tot, a_ms, tot, xms = [], [], [], []
                for _ in range(args.reps):  # (a) and (b) alternate
                    oeng.run_trials_sojourn(ocfgs, *sj_spec, groups=groups, ngroups=ngroups)
                    tm = oeng.timing()
                    a_tot.append(tm.total_ms); a_ms.append(tm.sojourn_ms)
                    res, _, x = eng.run_trials_xtab(cfgs, *spec, groups=groups, ngroups=ngroups)
                    tm = eng.timing()
                    tot.append(tm.total_ms); xms.append(tm.xtab_ms)
                got[scheme] = (a_tot, a_ms, tot, xms, x)
            assert got[0][4].same_as(got[1][4]), "the two schemes disagree"
            x = got[1][4]
            floor = bytes_per_ue[sname] * ues / HBM_BYTES_PER_MS
            c_ms, scheds = [], {}
            for rep in range(0 if args.no_host else 1):
                t0 = time.perf_counter()
                ref = np.zeros_like(x.cells)
                for lo in range(0, len(cfgs), args.slice):
                    part = cfgs[lo:lo + args.slice]
                    rr, logs = eng.run_trials(part, want_logs=True)
                    for k, lg in enumerate(logs):
                        c = part[k]
                        if (c.nUE, c.accessTime) not in scheds:
                            scheds[(c.nUE, c.accessTime)] = np.asarray(pkg.arrival_schedule(c)[0], dtype=np.int64)
                        ref[(lo + k) % 10 if groups else 0] += numpy_table(spec, np.frombuffer(lg, dtype=np.int32).reshape(-1, 16), scheds[(c.nUE, c.accessTime)], c.accessTime,
                                                                           min(rr[k].steps, rr[k].maxTime))
                c_ms.append(1e3 * (time.perf_counter() - t0))
                assert np.array_equal(ref, x.cells), "the two ways disagree"
            c_ms = c_ms or [float("nan")]
            for scheme in (0, 1):
                a_tot, a_ms, tot, xms, _ = got[scheme]
                main_rows.append(f"| {name} | {sname} | {sp(a_tot)} | {sp(a_ms, 3)} | {scheme} | {sp(tot)} | {sp(xms, 3)} | {med(tot) / med(a_tot):.3f} | {med(xms) / med(a_ms):.2f} | "
                                 f"{int(x.scalars['binned'].sum())} | {bytes_per_ue[sname]} | {floor:.4f} | {med(xms) / floor:.1f} | {med(c_ms):.0f} | {med(c_ms) / med(tot):.1f} |")
        if one_eng:  # (d) the two hot-cell binnings, alternating
            eng.set("xtab_scheme", 1)
            ccfgs = make(one)
            one_eng.run_trials_xtab(ccfgs, *specs["default"], groups=groups, ngroups=ngroups)
            four, single = [], []
            for _ in range(args.reps):
                _, _, x4 = eng.run_trials_xtab(cfgs, *specs["default"], groups=groups, ngroups=ngroups)
                four.append(eng.timing().xtab_ms)
                _, _, x1 = one_eng.run_trials_xtab(ccfgs, *specs["default"], groups=groups, ngroups=ngroups)
                single.append(one_eng.timing().xtab_ms)
            assert np.array_equal(x4.cells, x1.cells)
            copy_rows.append(f"| {name} | {sp(four, 3)} | {sp(single, 3)} | {med(single) / med(four):.2f} |")
    print("| workload | (p) parent sojourn total_ms (spread) | sojourn_ms (spread) |\n|---|---|---|")
    print("\n".join(spread_rows) + "\n")
    print("| workload | spec | (a) sojourn total_ms (spread) | sojourn_ms (spread) | scheme | (b) xtab total_ms (spread) | xtab_ms (spread) | (b) / (a) | xtab_ms / sojourn_ms | binned UEs | B per UE | byte floor (ms) | "
          "xtab_ms / floor | (c) logs + numpy (ms) | (c) / (b) |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(main_rows) + "\n")
    if copy_rows:
        print("| workload | per-wavefront copies: xtab_ms (spread) | one copy: xtab_ms (spread) | one copy / copies |\n|---|---|---|---|")
        print("\n".join(copy_rows))
    sys.stdout.flush()
    eng.close()
    if args.parent:
        oeng.close()
    if one_eng:
        one_eng.close()


if __name__ == "__main__":
    main()
