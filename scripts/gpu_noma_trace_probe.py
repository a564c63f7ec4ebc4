#!/usr/bin/env python3
"""scripts/gpu_noma_trace_probe.py [--reps N] [--other PKG_DIR ...] — what NOMA.c's channel trace costs, on one MI355X (profiles/noma_trace_kernel.md).

Every build named — this checkout's package first, then each --other (a package directory with its own __init__.py and libprach_hip.so: a checkout of the
parent commit, a second copy of it as the noise control, a variant build) — is loaded into ONE process and timed alternately, call by call, on NOMA.c's own
experiment (ten seeds x ten sweep points) and on the single 100 000-UE trial through plain prach_run_trials: kernel_ms per build.  The results of every build
are asserted equal, byte for byte.  Then, for this checkout: the traced call against its own plain call, alternating (kernel_ms, total_ms, noma_trace_ms)."""
import argparse
import importlib.util
import os
import statistics as st
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def workload(p, which):
    if which == "grid":
        return [p.make_cfg(n, variant=p.VARIANT_NOMA_C, rng_mode=p.RNG_PHILOX, seed=s) for s in range(10) for n in range(10000, 100001, 10000)]
    return [p.make_cfg(100000, variant=p.VARIANT_NOMA_C, rng_mode=p.RNG_PHILOX, seed=0)]


def line(tag, name, which, what, v):
    print(f"{tag} {name:40s} {which:5s} {what:14s} median {st.median(v):8.3f} min {min(v):8.3f} max {max(v):8.3f} n {len(v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--other", action="append", default=[])
    a = ap.parse_args()
    dirs = [os.path.join(ROOT, "5g-nr-randomaccess_amd")] + a.other
    pk = [load(d, f"prach_probe_{i}") for i, d in enumerate(dirs)]
    eng = [p.Engine(0) for p in pk]
    for which in ("grid", "one"):
        ref, ms = None, [[] for _ in dirs]
        for i in range(len(dirs)):  # warm-up of this shape, and the results for the comparison
            r, _ = eng[i].run_trials(workload(pk[i], which))
            ref = ref or [bytes(x) for x in r]
            assert [bytes(x) for x in r] == ref, (which, dirs[i])
        for _ in range(a.reps):
            for i in range(len(dirs)):
                eng[i].run_trials(workload(pk[i], which))
                ms[i].append(eng[i].timing().kernel_ms)
        for i, d in enumerate(dirs):
            line("PLAIN", os.path.relpath(d, ROOT), which, "kernel_ms", ms[i])
    e, p = eng[0], pk[0]
    for which in ("grid", "one"):
        c = workload(p, which)
        kw = dict(groups=[k % 10 for k in range(len(c))], ngroups=10) if len(c) > 1 else {}
        e.run_trials_noma_trace(c, 2000, 5, **kw)
        rows = {"plain_kernel": [], "plain_total": [], "traced_kernel": [], "traced_total": [], "noma_trace_ms": []}
        for _ in range(a.reps):
            e.run_trials(c)
            t = e.timing()
            rows["plain_kernel"].append(t.kernel_ms)
            rows["plain_total"].append(t.total_ms)
            e.run_trials_noma_trace(c, 2000, 5, **kw)
            t = e.timing()
            rows["traced_kernel"].append(t.kernel_ms)
            rows["traced_total"].append(t.total_ms)
            rows["noma_trace_ms"].append(t.noma_trace_ms)
        for k, v in rows.items():
            line("TRACED", "this checkout", which, k, v)
    for x in eng:
        x.close()


if __name__ == "__main__":
    main()
