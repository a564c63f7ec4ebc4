#!/usr/bin/env python3
"""scripts/gpu_noma_timeline_probe.py [--reps N] [--other PKG_DIR ...] — what NOMA.c's timeline costs, on one MI355X (profiles/noma_timeline_kernel.md).

Every build named — this checkout's package first, then each --other (a package directory with its own __init__.py and libprach_hip.so: a checkout of the
parent commit, a second copy of it as the noise control) — is loaded into ONE process and timed alternately, call by call, on NOMA.c's own experiment (ten
seeds x ten sweep points) and on the single 100 000-UE trial through plain prach_run_trials: kernel_ms per build.  The results of every build are asserted
equal, byte for byte.  Then, for this checkout, alternating: the plain call, the timeline call under both schemes and several window sizes
(noma_timeline_ms: the kernel alone; total_ms: the call), and the only other route to the same numbers — every log over the bus plus
noma_timeline_from_logs — whose result is asserted equal to the device's."""
import argparse
import importlib.util
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, BIN_MS = 2002, 5


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
    print(f"{tag} {name:40s} {which:5s} {what:18s} median {st.median(v):9.3f} min {min(v):9.3f} max {max(v):9.3f} n {len(v)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--windows", default="16,64,256,1024")
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
    setups = [(s, w) for s in (1,) for w in map(int, a.windows.split(","))] + [(0, 0)]
    for which in ("grid", "one"):
        c = workload(p, which)
        kw = dict(groups=[k % 10 for k in range(len(c))], ngroups=10) if len(c) > 1 else {}
        _, _, want = e.run_trials_noma_timeline(c, BINS, BIN_MS, **kw)
        rows = {"plain_kernel": [], "plain_total": []}
        for s, w in setups:
            rows[f"s{s}_w{w}_kernel"], rows[f"s{s}_w{w}_total"], rows[f"s{s}_w{w}_reducer"], rows[f"s{s}_w{w}_wall"] = [], [], [], []
        for _ in range(a.reps):
            e.run_trials(c)
            t = e.timing()
            rows["plain_kernel"].append(t.kernel_ms)
            rows["plain_total"].append(t.total_ms)
            for s, w in setups:
                e.set("timeline_scheme", s)
                e.set("noma_timeline_window", w)
                t0 = time.perf_counter()
                _, _, tl = e.run_trials_noma_timeline(c, BINS, BIN_MS, **kw)
                rows[f"s{s}_w{w}_wall"].append(1e3 * (time.perf_counter() - t0))  # (as the other route below is timed: the binding's work included)
                t = e.timing()
                assert tl.same_as(want), (which, s, w)
                rows[f"s{s}_w{w}_kernel"].append(t.kernel_ms)
                rows[f"s{s}_w{w}_total"].append(t.total_ms)
                rows[f"s{s}_w{w}_reducer"].append(t.noma_timeline_ms)
        e.set("timeline_scheme", 1)
        e.set("noma_timeline_window", 0)
        for k, v in rows.items():
            line("TIMELINE", "this checkout", which, k, v)
        host_call, host_def = [], []
        for _ in range(a.host_reps):  # the other route: every log over the bus, then the host definition
            t0 = time.perf_counter()
            res, logs = e.run_trials(c, want_logs=True)
            t1 = time.perf_counter()
            tl = p.noma_timeline_from_logs(c, [r.steps for r in res], logs, BINS, BIN_MS, **kw)
            t2 = time.perf_counter()
            assert tl.same_as(want), which
            host_call.append(1e3 * (t1 - t0))
            host_def.append(1e3 * (t2 - t1))
        line("HOST", "this checkout", which, "call_with_logs_ms", host_call)
        line("HOST", "this checkout", which, "from_logs_ms", host_def)
    for x in eng:
        x.close()


if __name__ == "__main__":
    main()
