"""The per-subframe preamble trace through every route of tests/tools/trace_cases.py, against the oracle (tests/tools/trace_ref.py).
usage: [PRACH_LIB=…/libprach_hip_nobitop3.so] gpu_trace_routes.py [--no-pin] [CASE …]   (--no-pin: a call is not held to its route's prach_timing pin)

Prints a line per route, then `done N routes B bad`; exit status 1 if B > 0.  tests/test_gpu_trace.py runs it in a child process with the library built
without v_bitop3 and with the small-queue build."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import __graft_entry__ as g
import trace_cases as TC
import trace_ref as TR


def main(args):
    pin = "--no-pin" not in args
    names = [a for a in args if a != "--no-pin"]
    pkg = g.load_package()
    eng = pkg.Engine(0)
    nbad = 0
    for route in TC.ROUTES:
        cases = TC.route_cases(route, names)
        TC.set_route(eng, route)
        bad, tm = TC.check_per_subframe(pkg, eng, cases, [TR.ref(c) for c in cases], pin=route if pin else None)
        nbad += bool(bad)
        print(f"route {route:<24} cases={len(cases):2d} rec_mode={tm.rec_mode} cluster_size={tm.cluster_size} fallback={tm.fallback_trials} {'ok' if not bad else 'BAD'}", flush=True)
        for b in bad[:10]:
            print("  " + b, flush=True)
    TC.reset(eng)
    eng.close()
    print(f"done {len(TC.ROUTES)} routes {nbad} bad  library {os.path.basename(pkg.LIB_PATH)}", flush=True)
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
