#!/usr/bin/env python3
"""scripts/gpu_noma_gain_probe.py [--reps N] [--other PKG_DIR ...] [--only-gain] — what NOMA.c's near-far profile costs, on one MI355X, and what it says
(profiles/noma_gain_kernel.md).

Every build named — this checkout's package first, then each --other (a package directory with its own __init__.py and libprach_hip.so: a checkout of the
parent commit, a second copy of it as the noise control) — is loaded into ONE process and timed alternately, call by call, on NOMA.c's own experiment (ten
seeds x ten sweep points) and on the single 100 000-UE trial through plain prach_run_trials: kernel_ms per build.  The results of every build are asserted
equal, byte for byte.  Then, for this checkout, alternating: the plain call, the gain call under both schemes at three bin counts — the default 65, the
largest the kernel keeps in LDS and one more (noma_gain_ms: the level pre-pass, the host's step and the reducer; total_ms: the call) — and the only other
route to the same numbers, every log over the bus plus noma_gain_from_logs, whose result is asserted equal to the device's.  (The two kernels apart:
rocprofv3 --kernel-trace --stats -- python scripts/gpu_noma_gain_probe.py --only-gain.)  Last, what the profile says about NOMA.c's seed 0 at 3000 UEs."""
import argparse
import importlib.util
import os
import statistics as st
import sys
import time

import numpy as np

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
    print(f"{tag} {name:40s} {which:5s} {what:22s} median {st.median(v):9.3f} min {min(v):9.3f} max {max(v):9.3f} n {len(v)}", flush=True)


def seed0(p, e):
    """NOMA.c's seed 0 at 3000 UEs through the device call: the ends of the gain axis, and where the stranded (STATE 5) UEs sit."""
    c = p.make_cfg(3000, variant=p.VARIANT_NOMA_C, rng_mode=p.RNG_PHILOX, seed=0)
    res, _, gn = e.run_trials_noma_gain([c])
    sc = {f: int(v[0]) for f, v in gn.scalars.items()}
    print(f"SEED0 served {sc['served']} dropped {sc['dropped']} pending {sc['pending']} idle {sc['idle']} undefined {sc['undefined']} below {sc['below']} above {sc['above']} "
          f"level_min {-sc['neg_level_max']} level_max {sc['level_max']} host_ues {e.timing().noma_gain_host_ues}")
    arr, sv, dr = gn.named("arrived", 0), gn.named("served", 0), gn.named("dropped", 0)
    occ = np.flatnonzero(arr > 0)
    ms = gn.mean_sojourn(0)
    for b in (occ[0], occ[-1]):
        print(f"SEED0 bin {int(gn.edges()[b])} .. {int(gn.edges()[b]) + gn.width - 1}: arrived {int(arr[b])} served {int(sv[b])} dropped {int(dr[b])} pending {int(arr[b] - sv[b] - dr[b])} "
              f"mean_sojourn_ms {ms[b]:.1f}")
    third = len(occ) // 3
    for name, bs in (("lowest third of the occupied bins", occ[:third]), ("middle third", occ[third:2 * third]), ("highest third", occ[2 * third:])):
        a, s, d = arr[bs].sum(), sv[bs].sum(), dr[bs].sum()
        print(f"SEED0 {name} ({int(gn.edges()[bs[0]])} .. {int(gn.edges()[bs[-1]]) + gn.width - 1}): arrived {int(a)} served {s / a:.4f} dropped {d / a:.4f} pending {(a - s - d) / a:.4f} "
              f"mean_sojourn_ms {gn.named('sojourn_sum', 0)[bs].sum() / s:.1f} mean_lost_ms {gn.named('lost_sum', 0)[bs].sum() / s:.1f} mean_ptc {gn.named('ptc_sum', 0)[bs].sum() / s:.2f}")
    _, _, col = e.run_trials_noma_columns([c], ["state"])
    lv = p.noma_gain_levels(c)
    stranded = np.sort(lv[col.trial(0)[0] == 5])
    print(f"SEED0 stranded (STATE 5) UEs: {len(stranded)}; levels {stranded.tolist()}; median {int(np.median(stranded)) if len(stranded) else None}; "
          f"median level of all arrived UEs {int(np.median(lv[col.trial(0)[0] != 0]))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--other", action="append", default=[])
    ap.add_argument("--only-gain", action="store_true")
    a = ap.parse_args()
    dirs = [os.path.join(ROOT, "5g-nr-randomaccess_amd")] + ([] if a.only_gain else a.other)
    pk = [load(d, f"prach_probe_{i}") for i, d in enumerate(dirs)]
    eng = [p.Engine(0) for p in pk]
    for which in (() if a.only_gain else ("grid", "one")):
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
    lds = p.noma_gain_lds_max_bins()
    specs = [(65, 200, -16200), (lds, 25, -16200), (lds + 1, 25, -16200)]
    setups = [(s, sp) for sp in specs for s in (1, 0)]
    for which in ("grid", "one"):
        c = workload(p, which)
        kw = dict(groups=[k % 10 for k in range(len(c))], ngroups=10) if len(c) > 1 else {}
        want = {sp: e.run_trials_noma_gain(c, *sp, **kw)[2] for sp in specs}
        rows = {"plain_kernel": [], "plain_total": []}
        for s, sp in setups:
            for what in ("kernel", "total", "gain", "wall", "host_ues"):
                rows[f"s{s}_b{sp[0]}_{what}"] = []
        for _ in range(a.reps):
            e.run_trials(c)
            t = e.timing()
            rows["plain_kernel"].append(t.kernel_ms)
            rows["plain_total"].append(t.total_ms)
            for s, sp in setups:
                e.set("timeline_scheme", s)
                t0 = time.perf_counter()
                _, _, gn = e.run_trials_noma_gain(c, *sp, **kw)
                rows[f"s{s}_b{sp[0]}_wall"].append(1e3 * (time.perf_counter() - t0))  # (as the other route below is timed: the binding's work included)
                t = e.timing()
                assert gn.same_as(want[sp]), (which, s, sp)
                rows[f"s{s}_b{sp[0]}_kernel"].append(t.kernel_ms)
                rows[f"s{s}_b{sp[0]}_total"].append(t.total_ms)
                rows[f"s{s}_b{sp[0]}_gain"].append(t.noma_gain_ms)
                rows[f"s{s}_b{sp[0]}_host_ues"].append(t.noma_gain_host_ues)
        e.set("timeline_scheme", 1)
        for k, v in rows.items():
            line("GAIN", "this checkout", which, k, v)
        host_call, host_def = [], []
        for _ in range(0 if a.only_gain else a.host_reps):  # the other route: every log over the bus, then the host definition
            t0 = time.perf_counter()
            res, logs = e.run_trials(c, want_logs=True)
            t1 = time.perf_counter()
            gn = p.noma_gain_from_logs(c, [r.steps for r in res], logs, *specs[0], **kw)
            t2 = time.perf_counter()
            assert gn.same_as(want[specs[0]]), which
            host_call.append(1e3 * (t1 - t0))
            host_def.append(1e3 * (t2 - t1))
        if host_call:
            line("HOST", "this checkout", which, "call_with_logs_ms", host_call)
            line("HOST", "this checkout", which, "from_logs_ms", host_def)
    seed0(p, e)
    for x in eng:
        x.close()


if __name__ == "__main__":
    main()
