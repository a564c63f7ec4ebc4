"""The kernel matrix on the GPU (tests/tools/kernel_matrix.py): every kernel with a compiler-chosen v_bitop3 table, pinned by engine options, at
the parameter corners where mask algebra goes wrong, judged trial by trial by the oracle.
usage: [PRACH_LIB=…/libprach_hip_nobitop3.so] gpu_kernel_matrix.py [--single] [ROW …]   (--single: every trial a call of its own)

Every trial against the oracle with tests/test_gpu_parity.py's assert_same bar (every KEYS counter, totalDelay, all 16 logged fields of every UE) or,
for NOMA.c, tests/test_noma.py's; every call's prach_timing against the row's pin (rec_mode, cluster_size) with no fallback trial and no rerun on
trial_kernel, so that a trial counts only if the kernel of its row produced it.  Prints a line per row with a digest of the results and logs, then
`done N cases B bad`; exit status 1 if B > 0.  Run with both libraries (tests/test_gpu_parity.py): a difference against the oracle that only the
shipped library shows points to the compiler's boolean instructions, one both show to the kernels' logic."""
import importlib.util
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import numpy as np

import __graft_entry__ as g
from oracle import binding as ob
from kernel_matrix import BETA_CASES, LEAVES, NOMA_CASES, RANDOM_CASES, ROWS

spec = importlib.util.spec_from_file_location("tgp", os.path.join(ROOT, "tests", "test_gpu_parity.py"))
tgp = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tgp)
pkg = g.load_package()

DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0)  # (every option a row sets, at the engine's defaults)
NOMA_UE = np.dtype([("i", np.int32, 16), ("g", np.float64)])


def batch_ok(n, kw):
    """prach_engine.hip batch_eligible for a case (the row's pin decides; this only keeps random cases the batch kernel cannot take out of its call)."""
    c = dict(nPreamble=54, backoff=20, maxRarWindow=6, accessTime=5, uniform=0)
    c.update(kw)
    need, slots = c["backoff"] + max(c["accessTime"], 5) + c["maxRarWindow"] + 70, 64
    while slots < need:
        slots *= 2
    return c["nPreamble"] <= 64 and c["maxRarWindow"] <= 11 and slots <= 256 and (60000 if c["uniform"] else 10000) + c["backoff"] + c["accessTime"] + 128 < 65000


def cases_of(row):
    """(program, variant, nUE, overrides, rng, seed) of every trial of a row (without those that leave its kernel by design: LEAVES)."""
    r = row["rng"]
    if row["program"] == "noma":
        return [("noma", 2, n, kw, r, s) for n, s, kw in NOMA_CASES]
    named = [(name, ("beta", v, n, kw, r, 100 * k + v)) for k, (name, n, kw) in enumerate(BETA_CASES) for v in (0, 1)]
    if row["random"]:
        rnd = [c for c in tgp._random_cases(4 * RANDOM_CASES, 20260 + r) if batch_ok(c[1], c[2])][:RANDOM_CASES]
        named += [(f"random_{s}", ("beta", v, n, kw, r, s)) for v, n, kw, _, s in rnd]
    return [c for name, c in named if row["name"] not in LEAVES.get(name, ())]


def key(c):
    return (c[0], c[1], c[2], tuple(sorted(c[3].items())), c[4], c[5])


def oracle(c):
    prog, v, n, kw, r, s = c
    if prog == "noma":
        okw = dict(kw)
        if "maxMsg2TxCount" in okw:
            okw["maxMsg1ReTx"] = okw.pop("maxMsg2TxCount")
        ocfg = ob.make_noma_cfg(n, **okw)
        return ocfg, ob.noma_run_trial(ocfg, ob.Rng(r, s))
    return None, ob.run_trial(ob.make_cfg(n, variant=v, **kw), ob.Rng(r, s))


def compare(c, res, logs, oc):
    """(failure text or None, the bytes the row's digest covers)."""
    prog, v, n, kw, r, s = c
    a = np.frombuffer(logs, dtype=np.int32).reshape(-1, 16)
    if prog == "noma":
        ocfg, (ores, oues) = oc
        b = np.frombuffer(oues, dtype=NOMA_UE)["i"]
        got = (res.status, res.nSuccessUE, res.sumTimer, res.preambleTxCount, res.failCounts, res.activeCheck, res.draws, res.time_exit)
        exp = (0, ores.nSuccessUE, ores.delay, ores.nTxP, ores.raFailedUEs, ores.activeCheck, ores.draws, ores.time_exit)
        if r == ob.RNG_GLIBC:  # (tests/test_noma.py's reference-stream bar counts the steps as well)
            got, exp = got + (res.steps,), exp + (ores.steps,)
        diff = np.where((a != b).any(axis=1))[0]
        why = None
        if got != exp:
            why = f"counters {got} != oracle {exp}"
        elif diff.size:
            why = f"{diff.size} UEs differ, first {diff[:5].tolist()}: {a[diff[0]].tolist()} != oracle {b[diff[0]].tolist()}"
        elif res.nSuccessUE and pkg.format_noma_line(pkg.make_cfg(n, variant=v, rng_mode=r, seed=s, **kw), res) != ob.noma_format_line(ocfg, ores):
            why = "result line differs"
        return why, struct.pack("<8q", *got[:8]) + a.tobytes()
    _, (ores, oues) = oc
    try:
        tgp.assert_same(pkg, res, logs, ores, oues, c)
        why = None
    except AssertionError as e:
        why = str(e)[:600]
    return why, struct.pack(f"<{len(tgp.KEYS)}qf", *[getattr(res, k) for k in tgp.KEYS], res.totalDelay) + a.tobytes()


def pin_failure(row, tm):
    want = dict(row["pin"], fallback_trials=0, trial_kernel_reruns=0)
    got = {k: getattr(tm, k) for k in want}
    return None if got == want else f"prach_timing {got}, the row pins {want}"


def main(names):
    single = "--single" in names  # (every trial a call of its own: names the trials that leave a row's kernel)
    names = [n for n in names if n != "--single"]
    rows = [r for r in ROWS if not names or r["name"] in names]
    assert rows, f"no row named {names}"
    t0 = time.time()
    cases = {}
    for row in rows:
        for c in cases_of(row):
            cases.setdefault(key(c), c)
    ob.lib()  # (loaded once before the threads: the oracle is plain C without global state, a call releases the GIL)
    nth = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)))
    with ThreadPoolExecutor(max_workers=nth) as ex:
        ref = dict(zip(cases, ex.map(oracle, cases.values())))
    print(f"oracle: {len(ref)} distinct trials in {time.time() - t0:.1f} s ({nth} threads)  library {os.path.basename(pkg.LIB_PATH)}", flush=True)
    eng = pkg.Engine(0)
    total = nbad = 0
    for row in rows:
        rc = cases_of(row)
        for k, v in DEFAULTS.items():
            eng.set(k, v)
        for k, v in row["opts"].items():
            eng.set(k, v)
        groups = [rc] if row["calls"] == "one_call" and not single else [[c] for c in rc]
        bad, digest, kms, t1 = set(), 0, 0.0, time.time()
        for grp in groups:
            cfgs = [pkg.make_cfg(n, variant=v, rng_mode=r, seed=s, **kw) for _, v, n, kw, r, s in grp]
            try:
                res, logs = eng.run_trials(cfgs, want_logs=True)
            except pkg.PrachError as e:
                print(f"  {row['name']}: call of {len(grp)} trials failed: {e}", flush=True)
                bad.update(key(c) for c in grp)
                continue
            tm = eng.timing()
            kms += tm.kernel_ms
            pf = pin_failure(row, tm)
            if pf:
                print(f"  {row['name']}: NOT PINNED {pf} ({len(grp)} trials, first {grp[0][1:]})", flush=True)
                bad.update(key(c) for c in grp)
                for c in grp if len(grp) > 1 else ():  # (which of them left the kernel: each alone)
                    eng.run_trials([pkg.make_cfg(c[2], variant=c[1], rng_mode=c[4], seed=c[5], **c[3])])
                    if pin_failure(row, eng.timing()):
                        print(f"  {row['name']}:   left by {c[1:]}: {pin_failure(row, eng.timing())}", flush=True)
            for c, rs_, lg in zip(grp, res, logs):
                why, blob = compare(c, rs_, lg, ref[key(c)])
                digest = zlib.crc32(blob, digest)
                if why:
                    print(f"  {row['name']}: MISMATCH {c[1:]}: {why}", flush=True)
                    bad.add(key(c))
        total += len(rc)
        nbad += len(bad)
        print(f"row {row['name']:<20} {'+'.join(row['kernels']):<45} cases={len(rc):3d} calls={len(groups):3d} bad={len(bad)} digest={digest:08x} "
              f"kernel={kms:.1f}ms wall={time.time() - t1:.2f}s", flush=True)
    for k, v in DEFAULTS.items():
        eng.set(k, v)
    eng.close()
    print(f"done {total} cases {nbad} bad ({time.time() - t0:.1f} s)", flush=True)
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
