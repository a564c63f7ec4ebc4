"""What the per-subframe preamble trace costs (prach_run_trials_trace, csrc/prach_trace.hip), on the three workloads of DESIGN.md 4: the 1000-trial Beta.c
grid, BASELINE config 3 (the same grid of RandomAccessWithNOMA) and one 100 000-UE trial.  Per workload, in ONE run, after a warm-up call of each kind, these
calls alternate `reps` times:
  (p1) (p2) plain prach_run_trials of the PARENT library (--parent DIR: the library built in that checkout, loaded next to this one), twice: the run-to-run
            spread of kernel_ms the parent shows against itself
  (a)       plain prach_run_trials of this library: the simulation kernels carry the trace's uniform branch and the call counter, and must stay inside that spread
  (b1) (b0) prach_run_trials_trace (bins of 5 ms over the horizon, ten groups) under trace_scheme 1 and 0: trace_ms, and the whole call against (a) — the
            per-subframe store and, on the single trial, the general cluster kernel in place of the lean one
and, beside trace_ms, the kernel's byte floor: 16 B per subframe and trial over 8 TB/s.  The two schemes must agree.  Prints one markdown table
(profiles/trace_kernel.md is this output).
usage: gpu_trace_probe.py [--reps 5] [--parent DIR] [--workloads grid,config3,single]"""
import argparse
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as g

HBM_BYTES_PER_MS = 8e9  # 8 TB/s


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
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    other = load_other(args.parent) if args.parent else pkg
    oeng = other.Engine(0) if args.parent else eng
    grid = lambda p, v: [p.make_cfg(n, variant=v, rng_mode=p.RNG_PHILOX, seed=s) for s in range(100) for n in range(10000, 100001, 10000)]
    work = {"grid": ("1000-trial Beta.c grid", lambda p: grid(p, p.VARIANT_BETA_C)), "config3": ("config 3 (1000 trials, RandomAccessWithNOMA)", lambda p: grid(p, p.VARIANT_WITHNOMA_C)),
            "single": ("one 100 000-UE trial (Beta.c)", lambda p: [p.make_cfg(100000, variant=p.VARIANT_BETA_C, rng_mode=p.RNG_PHILOX, seed=0)])}
    med = statistics.median
    sp = lambda v: f"{med(v):.2f} ({max(v) - min(v):.2f})"
    print(f"plain calls (p1), (p2) of: {'--parent ' + args.parent if args.parent else 'this checkout'}; reps {args.reps}; median (max - min)\n")
    print("| workload | (p1) parent kernel_ms | (p2) parent kernel_ms | (a) plain kernel_ms | (a) / (p1) | (a) plain total_ms | (b1) trace kernel_ms | (b1) trace total_ms | (b1) / (a) total | "
          "trace_ms scheme 1 | trace_ms scheme 0 | byte floor (ms) | scheme 1 / floor | rec_mode plain / trace |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, make = work[key]
        cfgs, ocfgs = make(pkg), make(other)
        groups = [k % 10 for k in range(len(cfgs))] if len(cfgs) > 1 else None
        ngroups = 10 if groups else 1
        oeng.run_trials(ocfgs)  # warm-up: the arena, the code objects
        eng.run_trials(cfgs)
        eng.set("trace_scheme", 1)
        eng.run_trials_trace(cfgs, 2000, 5, groups=groups, ngroups=ngroups)
        p1, p2, a_k, a_t, b_k, b_t, t1, t0 = [], [], [], [], [], [], [], []
        for _ in range(args.reps):
            oeng.run_trials(ocfgs); p1.append(oeng.timing().kernel_ms)
            oeng.run_trials(ocfgs); p2.append(oeng.timing().kernel_ms)
            res, _ = eng.run_trials(cfgs); tm = eng.timing(); a_k.append(tm.kernel_ms); a_t.append(tm.total_ms); rec_plain = tm.rec_mode
            eng.set("trace_scheme", 1)
            _, _, tr1 = eng.run_trials_trace(cfgs, 2000, 5, groups=groups, ngroups=ngroups); tm = eng.timing()
            b_k.append(tm.kernel_ms); b_t.append(tm.total_ms); t1.append(tm.trace_ms); rec_trace = tm.rec_mode
            eng.set("trace_scheme", 0)
            _, _, tr0 = eng.run_trials_trace(cfgs, 2000, 5, groups=groups, ngroups=ngroups); t0.append(eng.timing().trace_ms)
        eng.set("trace_scheme", 1)
        assert tr1.same_as(tr0), "the two schemes disagree"
        assert int(tr1.scalars["txop"].sum()) == sum(r.totalPreambleTxop for r in res) and int(tr1.scalars["collisions"].sum()) == sum(r.collisionPreambles for r in res)
        floor = 16 * sum(r.steps for r in res) / HBM_BYTES_PER_MS
        print(f"| {name} | {sp(p1)} | {sp(p2)} | {sp(a_k)} | {med(a_k) / med(p1):.4f} | {sp(a_t)} | {sp(b_k)} | {sp(b_t)} | {med(b_t) / med(a_t):.3f} | {med(t1):.3f} ({max(t1) - min(t1):.3f}) | "
              f"{med(t0):.3f} ({max(t0) - min(t0):.3f}) | {floor:.4f} | {med(t1) / floor:.1f} | {rec_plain} / {rec_trace} |", flush=True)
    eng.close()
    if args.parent:
        oeng.close()


if __name__ == "__main__":
    main()
