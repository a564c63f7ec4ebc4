"""What the NOMA census and the NOMA columns cost (prach_run_trials_noma_census, prach_run_trials_noma_columns; csrc/prach_noma_census.hip), on NOMA.c's own
experiment (ten seeds x the ten sweep points 10 000 .. 100 000 UEs, Philox: 100 trials, 5.5 M UEs) and on one 100 000-UE trial.  Per workload, in ONE run,
medians of repeated calls after a warm-up call, the spread (max - min over the repetitions) beside the median; (a), (b) and (c) alternate, and (d) runs
BEHIND them, in repetitions of its own (its 64 B per UE go to pageable host memory and would disturb the calls next to it):
  (a) the census call (the default table, arrival:500 x state:1:9, everybody): total_ms (the wall time of the call, which ends in a synchronise) and
      noma_census_ms (HIP events around the kernel), and the kernel's byte floor: 48 B read per UE (the quarters with class, txTime and nowBackoff) over 8 TB/s
  (b) the columns call with the host destination, fields state, arrival, sojourn, lost: total_ms and noma_columns_ms; floor: 64 B read + 16 B written per UE
  (c) plain prach_run_trials: total_ms and kernel_ms — what every route pays for the simulation itself
  (d) the only route without the two kinds: prach_run_trials with EVERY per-UE log plus the host definition (prach_noma_census_accumulate_logs /
      prach_noma_columns_from_logs) — wall time, host part included.  The probe asserts that its results equal (a)'s and (b)'s
Bytes over the bus per UE: (a) none (a table of 21 x 10 cells per group), (b) 4 per field, (d) 64.
Then the two findings on NOMA.c's seed 0, 3000 UEs, as the census prints them on the device.  Prints markdown (profiles/noma_census_kernel.md is this output).
usage: gpu_noma_census_probe.py [--reps 5] [--workloads grid,single]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as g  # noqa: E402

HBM_BYTES_PER_MS = 8e9  # 8 TB/s
FIELDS = ["state", "arrival", "sojourn", "lost"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="grid,single")
    args = ap.parse_args()
    pkg = g.load_package()
    eng = pkg.Engine(0)
    noma = lambda n, s: pkg.make_cfg(n, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=s)
    work = {"grid": ("NOMA.c's experiment (10 seeds x 10 points, 5.5 M UEs)", [noma(n, s) for s in range(10) for n in range(10000, 100001, 10000)], [k % 10 for k in range(100)]),
            "single": ("one 100 000-UE trial", [noma(100000, 0)], [0])}
    med = statistics.median
    sp = lambda v, d=2: f"{med(v):.{d}f} ({max(v) - min(v):.{d}f})"
    print(f"reps {args.reps}\n")
    print("| workload | (a) census: total_ms (spread) | noma_census_ms (spread) | floor (ms) | census_ms / floor | (b) columns: total_ms (spread) | noma_columns_ms (spread) | floor (ms) | "
          "columns_ms / floor | (c) plain: total_ms (spread) | kernel_ms (spread) | (d) logs + host census: ms (spread) | (d) / (a) | (d) logs + host columns: ms (spread) | (d) / (b) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for key in args.workloads.split(","):
        name, cfgs, groups = work[key]
        nue = sum(c.nUE for c in cfgs)
        eng.run_trials(cfgs)  # warm-up: the arena, the code objects
        eng.run_trials_noma_census(cfgs, groups=groups)
        eng.run_trials_noma_columns(cfgs, FIELDS)
        a_tot, a_k, b_tot, b_k, c_tot, c_k, d_cs, d_col = [], [], [], [], [], [], [], []
        for rep in range(args.reps):
            _, _, cs = eng.run_trials_noma_census(cfgs, groups=groups)
            tm = eng.timing()
            a_tot.append(tm.total_ms); a_k.append(tm.noma_census_ms)
            _, _, col = eng.run_trials_noma_columns(cfgs, FIELDS)
            tm = eng.timing()
            b_tot.append(tm.total_ms); b_k.append(tm.noma_columns_ms)
            eng.run_trials(cfgs)
            tm = eng.timing()
            c_tot.append(tm.total_ms); c_k.append(tm.kernel_ms)
        for rep in range(args.reps):  # (d), apart
            t0 = time.perf_counter()
            res, logs = eng.run_trials(cfgs, want_logs=True)
            hcs = pkg.noma_census_from_logs(cfgs, [r.steps for r in res], logs, groups=groups)
            d_cs.append(1e3 * (time.perf_counter() - t0))
            del logs
            t0 = time.perf_counter()
            res, logs = eng.run_trials(cfgs, want_logs=True)
            hcol = pkg.noma_columns_from_logs(cfgs, [r.steps for r in res], logs, FIELDS)
            d_col.append(1e3 * (time.perf_counter() - t0))
            del logs
            assert cs.same_as(hcs) and (col.data == hcol.data).all(), "the two routes disagree"
        fa, fb = 48 * nue / HBM_BYTES_PER_MS, (64 + 4 * len(FIELDS)) * nue / HBM_BYTES_PER_MS
        print(f"| {name} | {sp(a_tot)} | {sp(a_k, 3)} | {fa:.4f} | {med(a_k) / fa:.1f} | {sp(b_tot)} | {sp(b_k, 3)} | {fb:.4f} | {med(b_k) / fb:.1f} | {sp(c_tot)} | {sp(c_k)} | "
              f"{sp(d_cs, 0)} | {med(d_cs) / med(a_tot):.1f} | {sp(d_col, 0)} | {med(d_col) / med(b_tot):.1f} |", flush=True)

    # the findings, as the device prints them
    c = noma(3000, 0)
    _, _, st = eng.run_trials_noma_census([c], ("one", 1, 1), ("state", 1, 9))
    _, _, sj = eng.run_trials_noma_census([c], ("sojourn", 1, 1000), ("timer", 1, 1000), pkg.NOMA_WHO["served"])
    _, _, lost = eng.run_trials_noma_census([c], ("one", 1, 1), ("lost", 1, 1), pkg.NOMA_WHO["served"])
    _, _, age = eng.run_trials_noma_census([c], ("one", 1, 1), ("age", 1000, 10), pkg.NOMA_WHO["pending"])
    print("\nNOMA.c seed 0, 3000 UEs, 10 000 subframes (Philox), censused on the device:\n")
    print("| state | " + " | ".join(pkg.NOMA_STATE_NAMES) + " |\n|---|" + "---|" * 9)
    print("| UEs | " + " | ".join(str(int(v)) for v in st.cells[0, 0, :9]) + " |")
    print(f"\nserved {int(st.scalars['served'][0])}, pending {int(st.scalars['pending'][0])}, dropped {int(st.scalars['dropped'][0])}, idle {int(st.scalars['idle'][0])}; "
          f"every pending UE is in state 5 (stranded): {int(st.cells[0, 0, 5]) == int(st.scalars['pending'][0])}")
    print(f"served UEs that started over after a Msg3 timeout (LOST > 0): {int(lost.cells[0, 0, 1])}; the longest arrival-to-Msg4 time {int(sj.scalars['row_max'][0])} ms, "
          f"the longest logged timer {int(sj.scalars['col_max'][0])} ms")
    print(f"the largest AGE of a stranded UE (subframes since it arrived): {int(age.scalars['col_max'][0])}")
    eng.close()


if __name__ == "__main__":
    main()
