"""BASELINE config 5: the `--times` x nUE sweep sharded over the GPUs of one node.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \\
        5g-nr-randomaccess_amd/sweep.py --times 1000 --program beta --out results_dir

One process per GPU.  Philox trials are independent: they are dealt to ranks by descending cost
(`dist.shard_trials`), each rank runs its shard in ONE `prach_run_trials` call (one workgroup cluster per
trial), then ONE sum all-reduce (RCCL over xGMI; payload < 1 KB) merges the per-nUE aggregates and the
per-trial rows are gathered to rank 0, which writes `results.csv` with AveragePerformance.py's arithmetic
(sum of the per-seed 2-decimal values in seed order — not recoverable from the summed raw aggregates).
The reference runs the same grid serially (RandomAccessWithNOMA.c:216-221).
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--times", type=int, default=100)
    ap.add_argument("--program", choices=("beta", "withnoma"), default="beta")
    ap.add_argument("--sweep", default="10000:100000:10000")
    ap.add_argument("--out", default=".")
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--cdf", default=None, help="write the delay / preamble-count distributions of the successful UEs, one group per sweep point, to this CSV file")
    ap.add_argument("--cdf-bins", type=int, default=4096)
    ap.add_argument("--cdf-bin-ms", type=int, default=1)
    ap.add_argument("--timeline", default=None, help="write arrivals, successes, sojourn / timer sums by arrival time and completions by completion time, "
                    "one group per sweep point, to this CSV file (not together with --cdf)")
    ap.add_argument("--timeline-bin", type=int, default=5, help="width of a timeline bin in ms; the bins cover the horizon")
    ap.add_argument("--sojourn", default=None, help="write the histogram of the time from arrival to Msg4 by arrival row, one group per sweep point, to this CSV "
                    "file (not together with --cdf or --timeline)")
    ap.add_argument("--sojourn-arrival-ms", type=int, default=500, help="width of an arrival row in ms; the rows cover the arrivals")
    ap.add_argument("--sojourn-bin", type=int, default=5, help="width of a delay bin in ms; the bins cover the horizon")
    ap.add_argument("--ci", default=None, help="write mean, standard deviation, standard error, minimum and maximum ACROSS THE SEEDS of every sweep point — success "
                    "and restart ratio, mean sojourn / timer / preamble transmissions and their exact per-trial percentiles — to this CSV file (not together "
                    "with --cdf, --timeline or --sojourn)")
    ap.add_argument("--ci-levels", default="500,950,990", help="percentile levels in permille, at most 8")
    ap.add_argument("--trace", default=None, help="write the per-subframe preamble trace — preambles used (calls), decoded (singles), and what the programs add to "
                    "totalPreambleTxop and collisionPreambles, by time — one group per sweep point, to this CSV file (not together with --cdf, --timeline, "
                    "--sojourn or --ci)")
    ap.add_argument("--trace-bin", type=int, default=5, help="width of a trace bin in ms; the bins cover the horizon")
    ap.add_argument("--xtab", default=None, help="write the outcome cross-tabulation — by default what became of the UEs (idle, served, in a backoff, in a RAR "
                    "window, granted, waiting out a Msg3 timeout) by when they arrived — one group per sweep point, to this CSV file (not together with --cdf, "
                    "--timeline, --sojourn, --ci or --trace)")
    ap.add_argument("--xtab-rows", default="arrival:500", help="FIELD[:WIDTH[:BINS]], FIELD one of one, arrival, sojourn, completion, timer, ptc, failcount, age, state")
    ap.add_argument("--xtab-cols", default="state:1:7", help="FIELD[:WIDTH[:BINS]]")
    ap.add_argument("--xtab-who", default="all", choices=("served", "unserved", "arrived", "all"), help="the UEs that enter the table")
    ap.add_argument("--pick", default=None, help="write WHICH UEs stand behind a count: per trial, in trial order, a header line with the exact number of matches and "
                    "the K UEs that pass every --pick-where clause — the first K by index, or those with the largest (--pick-top) / smallest (--pick-bottom) FIELD — "
                    "to this CSV file (not together with --cdf, --timeline, --sojourn, --ci, --trace or --xtab)")
    ap.add_argument("--pick-where", action="append", default=[], help="FIELD:LO:HI, LO <= FIELD <= HI; at most 4; FIELD as for --xtab-rows")
    ap.add_argument("--pick-top", default=None, help="FIELD: the K UEs with the largest value")
    ap.add_argument("--pick-bottom", default=None, help="FIELD: the K UEs with the smallest value")
    ap.add_argument("--pick-k", type=int, default=16, help="UEs per trial, 1 to 4096")
    ap.add_argument("--pick-who", default="all", choices=("served", "unserved", "arrived", "idle", "all"), help="the UEs that are selected")
    ap.add_argument("--same-device", action="store_true", help="rehearsal on one GPU: every rank uses cuda:0")
    args = ap.parse_args(argv)
    if args.cdf and args.timeline:
        ap.error("--cdf and --timeline cannot be combined: one reduction per call")
    if args.sojourn and (args.cdf or args.timeline):
        ap.error("--sojourn cannot be combined with --cdf or --timeline: one reduction per call")
    if args.ci and (args.cdf or args.timeline or args.sojourn):
        ap.error("--ci cannot be combined with --cdf, --timeline or --sojourn: one reduction per call")
    if args.trace and (args.cdf or args.timeline or args.sojourn or args.ci):
        ap.error("--trace cannot be combined with --cdf, --timeline, --sojourn or --ci: one reduction per call")
    if args.xtab and (args.cdf or args.timeline or args.sojourn or args.ci or args.trace):
        ap.error("--xtab cannot be combined with --cdf, --timeline, --sojourn, --ci or --trace: one reduction per call")
    if args.pick and (args.cdf or args.timeline or args.sojourn or args.ci or args.trace or args.xtab):
        ap.error("--pick cannot be combined with --cdf, --timeline, --sojourn, --ci, --trace or --xtab: one reduction per call")
    if args.pick_top and args.pick_bottom:
        ap.error("--pick-top FIELD or --pick-bottom FIELD: one of them")
    ci_levels = [int(x) for x in args.ci_levels.split(",")]
    if not 1 <= len(ci_levels) <= 8 or any(m < 1 or m > 1000 for m in ci_levels):
        ap.error("--ci-levels takes 1 to 8 levels between 1 and 1000")

    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    distmod = importlib.import_module(pkg.__name__ + ".dist")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.same_device else int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    lo, hi, step = map(int, args.sweep.split(":"))
    points = list(range(lo, hi + 1, step))
    variant = pkg.VARIANT_BETA_C if args.program == "beta" else pkg.VARIANT_WITHNOMA_C
    cfgs = [pkg.make_cfg(n, variant=variant, rng_mode=pkg.RNG_PHILOX, seed=s) for s in range(args.times) for n in points]
    mine = distmod.shard_trials(cfgs, rank, world)

    eng = pkg.Engine(local_rank)
    t0 = time.perf_counter()
    res = []
    CH = 1024  # trials per call: bounds the device arena (2.7 GB per 1024 trials of the sweep)
    tl_bins = -(-(10000 + 6) // args.timeline_bin)  # Beta arrivals: 10 000 subframes, a completion at most 6 behind
    # the sweep's reduction, one group per sweep point: its accumulator, the engine call that makes a chunk's and its leading arguments, then the
    # all-reduce across ranks, the CSV formatter and the file
    red = None
    if args.cdf:
        red = (pkg.Dist(len(points), args.cdf_bins, args.cdf_bin_ms), eng.run_trials_dist, (args.cdf_bins, args.cdf_bin_ms), distmod.allreduce_dist, pkg.dist_csv, args.cdf)
    elif args.timeline:
        red = (pkg.Timeline(len(points), tl_bins, args.timeline_bin), eng.run_trials_timeline, (tl_bins, args.timeline_bin), distmod.allreduce_timeline, pkg.timeline_csv, args.timeline)
    elif args.sojourn:
        sj = (-(-10000 // args.sojourn_arrival_ms), args.sojourn_arrival_ms, -(-(10000 + 6) // args.sojourn_bin), args.sojourn_bin)
        red = (pkg.Sojourn(len(points), *sj), eng.run_trials_sojourn, sj, distmod.allreduce_sojourn, pkg.sojourn_csv, args.sojourn)
    elif args.trace:
        tr_bins = -(-10000 // args.trace_bin)  # Beta arrivals: 10 000 subframes
        red = (pkg.Trace(len(points), tr_bins, args.trace_bin), eng.run_trials_trace, (tr_bins, args.trace_bin), distmod.allreduce_trace, pkg.trace_csv, args.trace)
    elif args.xtab:
        try:
            xa = (pkg.xtab_parse_axis(args.xtab_rows, 10000), pkg.xtab_parse_axis(args.xtab_cols, 10000), pkg.XTAB_WHO[args.xtab_who])
        except ValueError as err:
            ap.error(str(err))
        red = (pkg.Xtab(len(points), *xa), eng.run_trials_xtab, xa, distmod.allreduce_xtab, pkg.xtab_csv, args.xtab)
    pick = None
    if args.pick:
        try:
            pick = dict(where=[pkg.pick_parse_clause(t) for t in args.pick_where], order="largest" if args.pick_top else "smallest" if args.pick_bottom else "index",
                        key=args.pick_top or args.pick_bottom, k=args.pick_k, who=pkg.XTAB_WHO[args.pick_who])
            if pick["key"] is not None and pick["key"].lower() not in pkg.XTAB_FIELD_NAMES:
                raise ValueError(f"--pick-top / --pick-bottom FIELD, one of {', '.join(pkg.XTAB_FIELD_NAMES)}: {pick['key']!r}")
        except ValueError as err:
            ap.error(str(err))
    ci_rows, pick_parts = [], []
    for a in range(0, len(mine), CH):
        part = mine[a:a + CH]
        if args.ci:  # one row per trial comes from the device with the results
            r, _, sm = eng.run_trials_summary([cfgs[i] for i in part], ci_levels)
            ci_rows.append(sm.rows)
        elif pick:  # the headers and rows of the chunk's trials come from the device with the results
            r, _, pk = eng.run_trials_pick([cfgs[i] for i in part], **pick)
            pick_parts.append(pk)
        elif red is None:
            r, _ = eng.run_trials([cfgs[i] for i in part])
        else:  # the chunk's reduction comes from the device with the results: no per-UE log is copied
            acc, run, params = red[:3]
            r, _, got = run([cfgs[i] for i in part], *params, groups=[i % len(points) for i in part], ngroups=len(points))
            for k in range(len(points)):
                acc.merge_group(k, got, k)
        res.extend(r)
    dt = time.perf_counter() - t0
    agg = distmod.aggregate_rows([cfgs[i] for i in mine], res, points)
    tot = distmod.allreduce_aggregates(agg, device=dev if (world > 1 and args.backend == "nccl") else None)
    # per-trial Results.txt texts (Beta.c's six lines; latency 0) travel to rank 0 for the exact results.csv — only where they are
    # consumed: AveragePerformance.py reads the Beta.c program's files
    allrows = None
    if variant == pkg.VARIANT_BETA_C:
        rows = [(i, pkg.format_results(cfgs[i], r, 0.0).decode()) for i, r in zip(mine, res)]
        allrows = distmod.gather_trial_rows(rows, dst=0, device=dev if (world > 1 and args.backend == "nccl") else None)
    if red is not None:
        acc, _, _, allreduce, to_csv, path = red
        allreduce(acc, device=dev if (world > 1 and args.backend == "nccl") else None)
        if rank == 0:
            with open(path, "wb") as f:
                f.write(to_csv(acc, labels=points))
    if args.ci:  # the rows travel to rank 0 and are put in trial order there: the statistics do not depend on the number of ranks
        import numpy as np
        mine_rows = np.concatenate(ci_rows) if ci_rows else np.zeros(0, dtype=pkg.summary_row_dtype())
        every = distmod.gather_summary_rows(mine_rows, mine, dst=0, device=dev if (world > 1 and args.backend == "nccl") else None)
        if rank == 0:
            sm = pkg.Summary(len(cfgs), ci_levels)
            sm.rows[:] = every
            with open(args.ci, "wb") as f:
                f.write(pkg.summary_csv(sm, groups=[i % len(points) for i in range(len(cfgs))], ngroups=len(points), labels=points))
    if pick:  # the trials travel to rank 0 and are put in trial order there: the file does not depend on the number of ranks
        import numpy as np
        every = pkg.Pick(len(cfgs), **pick)
        heads = np.concatenate([p.headers for p in pick_parts]) if pick_parts else every.headers[:0]
        rows = np.concatenate([p.rows for p in pick_parts]) if pick_parts else every.rows[:0]
        got = distmod.gather_pick_rows(heads, rows, mine, dst=0, device=dev if (world > 1 and args.backend == "nccl") else None)
        if rank == 0:
            every.headers[:], every.rows[:] = got
            with open(args.pick, "wb") as f:
                f.write(pkg.pick_csv(every, cfgs))
    if rank == 0:
        fi = {n: k for k, n in enumerate(distmod.AGG_FIELDS)}
        summary = {"program": args.program, "times": args.times, "points": points, "world": world,
                   "updates": int(tot[:, fi["updates"]].sum()), "rank0_seconds": dt,
                   "success_ratio": {str(p): float(tot[k, fi["nSuccessUE"]]) / (args.times * p) for k, p in enumerate(points)}}
        if variant == pkg.VARIANT_BETA_C:
            by = dict(allrows)
            per_point = [[by[s * len(points) + k] for s in range(args.times)] for k in range(len(points))]
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, "results.csv"), "wb") as f:
                f.write(pkg.results_csv(per_point))
            summary["results_csv"] = os.path.join(args.out, "results.csv")
        print(json.dumps(summary), flush=True)
    eng.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
