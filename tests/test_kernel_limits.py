"""Every kernel-selection limit of the engine from both sides (tests/tools/kernel_limits.py).

The engine picks a kernel per launch by hard limits of the kernels (a table stride, a 16-bit subframe number, a 20-bit UE index, a group table in LDS),
each restated by hand in two or three places.  An off-by-one there is no crash: it is a silent rerun on a slower kernel or a truncated field.  The GPU
test runs every case of the table on its last value inside and its first outside, bit-exact against the oracle, and asserts the kernel the engine's
source predicts on each side; the CPU tests prove from the oracle alone that every case stands where the table says.

Wall time, measured: the CPU tests 82 s on 8 cores (the oracle's calls, 151 s of CPU time), the GPU test 112 s on the MI355X box (83 s of them the
oracle's calls on 8 threads; the 72 GPU calls take 28 s, 14 s of that the 1 100 000-UE trial of 8 000 subframes on trial_kernel) — against 395 s for the
whole GPU suite before it."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
try:
    import kernel_limits as kl
finally:
    sys.path.pop(0)

EXACT = [c for c in kl.CASES if c["expect"] == "exact"]
TIMEOUT_GPU = 350  # seconds: three times the measured run


def _oracle_cfg(ob, c):
    if c["variant"] == kl.NOMA:
        kw = dict(c["kw"])
        if "maxMsg2TxCount" in kw:
            kw["maxMsg1ReTx"] = kw.pop("maxMsg2TxCount")
        return ob.make_noma_cfg(c["nUE"], **kw)
    return ob.make_cfg(c["nUE"], variant=c["variant"], **c["kw"])


def _facts(ob, c):
    """What the oracle alone says about a case: counters, the largest txTime of its log, UEs still under way at the end, the highest index that left idle."""
    cfg = _oracle_cfg(ob, c)
    if c["variant"] == kl.NOMA:
        res, ues = ob.noma_run_trial(cfg, ob.Rng(c["rng"], c["seed"]))
        a = np.frombuffer(ues, dtype=np.dtype([("i", np.int32, 16), ("g", np.float64)]))["i"]
        f = dict(success=res.nSuccessUE, activeCheck=res.activeCheck, draws=res.draws, time_exit=res.time_exit, steps=res.steps)
    else:
        res, ues = ob.run_trial(cfg, ob.Rng(c["rng"], c["seed"]))
        a = np.frombuffer(ues, dtype=np.int32).reshape(-1, 16)
        f = dict(success=res.nSuccessUE, activeCheck=res.activeCheck, draws=res.draws, time_exit=res.time_exit, steps=res.steps)
    active, tx = a[:, 2], a[:, 3]  # (UE_FIELDS: idx, timer, active, txTime, ...)
    f["max_tx"] = int(tx.max())
    f["under_way"] = int((active > 0).sum())
    arrived = np.nonzero(active != -1)[0]
    f["top_index"] = int(arrived[-1]) if arrived.size else -1
    return f


@pytest.fixture(scope="module")
def facts(ob):
    ob.lib()
    distinct = {}
    for c in EXACT:
        distinct.setdefault((c["variant"], c["nUE"], tuple(sorted(c["kw"].items())), c["rng"], c["seed"]), c)
    order = sorted(distinct, key=lambda k: -k[1] * (dict(k[2]).get("max_steps") or 10000))
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        out = dict(zip(order, ex.map(lambda k: _facts(ob, distinct[k]), order)))
    return {c["name"]: out[(c["variant"], c["nUE"], tuple(sorted(c["kw"].items())), c["rng"], c["seed"])] for c in EXACT}


def test_table_names_every_limit_of_the_device_header():
    """Every limit function / constant prach_device.h exports for the engine's kernel choice has an entry: a new limit without one fails here."""
    with open(os.path.join(ROOT, "5g-nr-randomaccess_amd", "csrc", "prach_device.h")) as f:
        text = re.sub(r"//.*", "", f.read())
    exported = set(re.findall(r"\b(batch_max_\w+|lcluster_max_\w+|batch_calendar_slots|CLUSTER_LQCAP|CLUSTER_GLIBC_MAX_UE)\b", text))
    assert len(exported) >= 10, exported
    covered = {n for lim in list(kl.LIMITS.values()) + list(kl.UNREACHABLE.values()) for n in lim["covers"]}  # (a clause no configuration reaches: on record as such)
    assert not exported - covered, f"limits of prach_device.h without an entry in tests/tools/kernel_limits.py: {sorted(exported - covered)}"
    assert not (covered & {"batch_max_preambles", "CLUSTER_LQCAP"}) - exported  # (the pattern still finds them)


def test_every_limit_has_an_unexcused_case_on_both_sides():
    """Each limit: at least one case inside and one outside that may not leave its kernel; LEAVES excuses at most one case in eight."""
    names = [c["name"] for c in kl.CASES]
    assert len(names) == len(set(names))
    assert set(kl.LEAVES) <= set(names) and 8 * len(kl.LEAVES) <= len(kl.CASES) and set(kl.MEASURED) <= set(names) | {kl.MIXED_CALL["name"]}
    for lim in kl.LIMITS:
        for side in ("in", "out"):
            firm = [c for c in kl.CASES if c["limit"] == lim and c["side"] == side and c["name"] not in kl.LEAVES]
            assert firm, f"limit {lim}: no case on the side {side!r} that must stay on its kernel"
            for c in firm:
                if c["expect"] == "exact":
                    assert c["pin"]["fallback_trials"] == 0 and c["pin"]["trial_kernel_reruns"] == 0 and "cluster_size" in c["pin"], c["name"]
    assert {c["limit"] for c in kl.CASES} == set(kl.LIMITS)
    assert any(n >= (1 << 20) - 1 for _, n, _, _ in kl.MIXED_CALL["trials"]) and any(n < 100000 for _, n, _, _ in kl.MIXED_CALL["trials"])


def test_cases_stand_on_the_values_the_table_states():
    """The parameter that decides each limit takes the table's inside / outside value in the cases of that side (computed as the engine computes it)."""
    for c in kl.CASES:
        lim, kw, want = kl.LIMITS[c["limit"]], c["kw"], None
        want = lim["inside"] if c["side"] == "in" else lim["outside"]
        if c["limit"] in ("batch_preambles", "lcluster_preambles", "noma_preambles"):
            assert kw["nPreamble"] == want, c["name"]
        elif c["limit"] == "batch_rar_window":
            assert kw["maxRarWindow"] == want, c["name"]
        elif c["limit"] in ("calendar_128_256", "calendar_256_leave"):
            need = kw.get("backoff", 20) + max(kw.get("accessTime", 5), 5) + kw.get("maxRarWindow", 6) + 70
            assert need == c["pre"]["need"] == want, (c["name"], need)
        elif c["limit"] == "compact_record":
            assert kw["uniform"] == 1 and kw["backoff"] + kw.get("accessTime", 5) == want, c["name"]
            assert (60000 + want + 64 < 63000) == (c["side"] == "in")
        elif c["limit"] in ("glibc_batch_groups", "glibc_cluster_size"):
            assert c["nUE"] == want and c["rng"] == kl.GLIBC, c["name"]
        elif c["limit"] in ("lds_slots_philox", "lds_slots_general", "lds_slots_glibc"):
            g = c["opts"]["cluster"]
            slots = ((c["nUE"] + 63) // 64 + g - 1) // g * 64  # (lds_record_slots)
            assert slots == want and (c["rng"] == kl.GLIBC) == (c["limit"] == "lds_slots_glibc"), (c["name"], slots)
        elif c["limit"] == "ue_index_20bit":
            assert (c["nUE"] <= lim["inside"]) == (c["side"] == "in"), c["name"]
        elif c["limit"] == "largest_size":
            assert c["nUE"] == want, c["name"]
    assert any(c["limit"] == "calendar_128_256" and c["kw"].get("accessTime", 5) > 5 for c in kl.CASES)
    assert any(c["limit"] == "ue_index_20bit" and c["nUE"] == 1048576 for c in kl.CASES)
    for lim in ("lds_slots_philox", "lds_slots_glibc"):
        assert {c["opts"]["cluster"] for c in kl.CASES if c["limit"] == lim} == {16, 32}, lim
    for c in kl.CASES:  # (the measured pins on file are those the entries expect)
        if c["name"] in kl.LEAVES or c["name"] not in kl.MEASURED:
            continue
        m = kl.MEASURED[c["name"]]
        assert m == "PRACH_ERR_UNSUPPORTED" if c["expect"] == "unsupported" else all(f"{k}={v}" in m.split() for k, v in c["pin"].items()), (c["name"], m)


def test_lds_limits_are_the_library_s_own(pkg):
    """The slot counts of the two LDS limits, from the library's own size functions (host code: no GPU): which condition binds, as the table says."""
    import ctypes as C
    L = C.CDLL(pkg.LIB_PATH)
    lean, gen = L._ZN5prach25lcluster_kernel_lds_bytesEibi, L._ZN5prach24cluster_kernel_lds_bytesEibi
    for f in (lean, gen):
        f.restype, f.argtypes = C.c_size_t, [C.c_int, C.c_bool, C.c_int]
    limit = 160 * 1024  # CLUSTER_LDS_LIMIT
    p = kl.LIMITS["lds_slots_philox"]
    assert lean(p["inside"], False, 0) <= limit < lean(p["outside"], False, 0) and p["inside"] < 4096  # (the LDS-byte test binds, not CLUSTER_LQCAP)
    q = kl.LIMITS["lds_slots_general"]
    assert gen(64, False, q["inside"]) <= limit < gen(64, False, q["outside"]) and q["inside"] < 4096
    g = kl.LIMITS["lds_slots_glibc"]
    assert lean(g["inside"], True, g["inside"] * 16 // 64) <= limit and g["inside"] == 4096  # (CLUSTER_LQCAP binds: the bytes would admit more)
    assert lean(g["outside"], True, g["outside"] * 16 // 64) <= limit
    assert lean(g["inside"], True, g["inside"] * 32 // 64) <= limit and lean(g["outside"], True, g["outside"] * 32 // 64) <= limit  # (32 workgroups: the same)
    assert lean(4096, True, 4096) > limit  # (lcluster_max_groups_glibc() groups in CLUSTER_LQCAP slots: 64 workgroups, never admitted)
    for name, val in (("_ZN5prach19batch_max_preamblesEv", 64), ("_ZN5prach20batch_max_rar_windowEv", 11), ("_ZN5prach24batch_max_calendar_slotsEv", 256),
                      ("_ZN5prach22lcluster_max_preamblesEv", 64), ("_ZN5prach25lcluster_max_groups_glibcEv", 4096), ("_ZN5prach19batch_max_subframesEv", 65000)):
        assert getattr(L, name)() == val, name
    bg = L._ZN5prach16batch_max_groupsEb
    bg.argtypes = [C.c_bool]
    assert bg(True) * 64 == kl.LIMITS["glibc_batch_groups"]["inside"] and bg(False) * 64 == 1 << 20


def test_oracle_places_every_case(facts):
    """The oracle alone: the Uniform cases run to subframe 60 000 with UEs still under way; the cases past 16 bits have a txTime >= 65 536 in the log and the
    compact ones stay below; the large cases have arrivals, successes and draws, and the long one puts UEs with an index past 2^20 under way."""
    for c in EXACT:
        f, pre = facts[c["name"]], c["pre"]
        assert f["draws"] > 0 and f["activeCheck"] > 0 and f["success"] > 0, (c["name"], f)
        if pre.get("uniform_runs_out"):
            assert c["kw"]["uniform"] == 1 and f["steps"] == 60000 and f["time_exit"] >= 59999 and f["under_way"] > 0, (c["name"], f)
        if "tx_at_least" in pre:
            assert f["max_tx"] >= pre["tx_at_least"], (c["name"], f)
        if "tx_below" in pre:
            assert 60000 < f["max_tx"] < pre["tx_below"], (c["name"], f)
        if "index_past" in pre:
            assert f["top_index"] >= pre["index_past"] and f["under_way"] > 0, (c["name"], f)
        if c["limit"] == "subframe_16bit" or c["limit"] == "compact_record":
            assert pre.get("uniform_runs_out"), c["name"]


@pytest.mark.gpu
def test_gpu_every_limit_from_both_sides(pkg):
    """tests/tools/gpu_kernel_limits.py once, in a child process: 0 bad, and every case reported — with the pin the table expects on its side, or the
    PRACH_ERR_UNSUPPORTED it expects."""
    runner = os.path.join(ROOT, "tests", "tools", "gpu_kernel_limits.py")
    env = dict(os.environ)
    env.pop("PRACH_LIB", None)
    p = subprocess.run([sys.executable, runner], env=env, capture_output=True, text=True, timeout=TIMEOUT_GPU)
    print(p.stdout)
    lines = {l.split()[1]: l for l in p.stdout.split("\n") if l.startswith("case ")}
    assert p.returncode == 0 and " cases 0 bad" in p.stdout and "ENDED EARLY" not in p.stdout, (p.stdout[-6000:], p.stderr[-3000:])
    for c in kl.CASES:
        line = lines.get(c["name"])
        assert line and " ok " in line, (c["name"], line)
        if c["expect"] == "unsupported":
            assert "status=-2" in line, line
        elif c["name"] not in kl.LEAVES:
            for k, v in c["pin"].items():
                assert f" {k}={v} " in line, (c["name"], k, v, line)
    assert kl.MIXED_CALL["name"] in lines and " ok " in lines[kl.MIXED_CALL["name"]]
    assert f"done {len(kl.CASES) + 1} cases 0 bad" in p.stdout
