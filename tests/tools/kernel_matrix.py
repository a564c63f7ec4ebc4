"""The kernel matrix: which engine options pin which kernel, and which kernels the GPU cross-check covers.

tests/tools/gpu_kernel_matrix.py runs every row on the GPU against the oracle (with libprach_hip.so and with libprach_hip_nobitop3.so,
tests/test_gpu_parity.py); tests/test_isa_bitop3.py reads COVERAGE without a GPU: every kernel of the library with a compiler-chosen
v_bitop3 truth table (scripts/isa_bitop3.py) must be pinned by a row here.  Plain data: no GPU, no oracle, no package import."""

# A row: the program ("beta": Beta.c and RandomAccessWithNOMA, both variants; "noma": NOMA.c), the RNG mode (0: the reference's rand() stream,
# 1: Philox), the engine options, whether every case is a call of its own ("single") or all cases share one call ("one_call"), and the
# prach_timing fields every call must report (fallback_trials == 0 and trial_kernel_reruns == 0 are asserted for every row).
ROWS = [
    dict(name="batch_w8_philox", kernels=["batch_kernel<8, false>"], program="beta", rng=1,
         opts=dict(cluster=1, batch_waves=8), calls="one_call", random=True, pin=dict(rec_mode=4, cluster_size=1)),
    dict(name="batch_w16_philox", kernels=["batch_kernel<16, false>"], program="beta", rng=1,
         opts=dict(cluster=1, batch_waves=16), calls="one_call", random=True, pin=dict(rec_mode=4, cluster_size=1)),
    dict(name="batch_glibc", kernels=["batch_kernel<16, true>"], program="beta", rng=0,
         opts=dict(cluster=1), calls="one_call", random=True, pin=dict(rec_mode=4, cluster_size=1)),
    dict(name="lcluster4_philox", kernels=["lcluster_kernel<false>"], program="beta", rng=1,
         opts=dict(cluster=4), calls="single", random=False, pin=dict(rec_mode=3, cluster_size=4)),
    dict(name="lcluster16_philox", kernels=["lcluster_kernel<false>"], program="beta", rng=1,
         opts=dict(cluster=16), calls="single", random=False, pin=dict(rec_mode=3, cluster_size=16)),
    dict(name="lcluster4_glibc", kernels=["lcluster_kernel<true>"], program="beta", rng=0,
         opts=dict(cluster=4), calls="single", random=False, pin=dict(rec_mode=3, cluster_size=4)),
    dict(name="lcluster16_glibc", kernels=["lcluster_kernel<true>"], program="beta", rng=0,
         opts=dict(cluster=16), calls="single", random=False, pin=dict(rec_mode=3, cluster_size=16)),
    # 16-byte records with one workgroup per trial: not the batch kernel (wide_records), not the compact 8 + 4 byte layout
    dict(name="cluster_wide_glibc", kernels=["cluster_kernel<true, 0>"], program="beta", rng=0,
         opts=dict(cluster=1, wide_records=1), calls="one_call", random=False, pin=dict(rec_mode=0, cluster_size=1)),
    dict(name="noma1_philox", kernels=["noma_kernel", "noma_activation_kernel"], program="noma", rng=1,
         opts=dict(cluster=1), calls="one_call", random=False, pin=dict(cluster_size=1)),
    dict(name="noma4_philox", kernels=["noma_kernel", "noma_activation_kernel"], program="noma", rng=1,
         opts=dict(cluster=4), calls="one_call", random=False, pin=dict(cluster_size=4)),
    # (the single-launch form: a trial it hands to the host-activated form is a fallback trial; the finishing kernel runs behind either form)
    dict(name="noma_glibc", kernels=["noma_glibc_trial_kernel", "noma_glibc_finish_kernel"], program="noma", rng=0,
         opts=dict(), calls="one_call", random=False, pin=dict()),
    # trial_kernel has only the Philox xor3 table; a cheap row all the same (cluster_size 0: the one-workgroup trial kernel)
    dict(name="legacy_philox", kernels=["trial_kernel<false>"], program="beta", rng=1,
         opts=dict(legacy=1), calls="one_call", random=False, pin=dict(cluster_size=0)),
]

# kernel symbol (as scripts/isa_bitop3.py names it) -> the rows that pin it
COVERAGE = {}
for _r in ROWS:
    for _k in _r["kernels"]:
        COVERAGE.setdefault(_k, []).append(_r["name"])

# Beta.c / RandomAccessWithNOMA cases (name, nUE, overrides), each for both variants.  The corner the ROCm 7.2 miscompile lived in (LABNOTES,
# round 4) comes first: no Msg2 retransmission allowed, one UL grant, a one-subframe RAR window.
BETA_CASES = [
    ("corner_1500", 1500, dict(maxMsg2TxCount=0, nGrantUL=1, maxRarWindow=1)),
    ("corner_5000", 5000, dict(maxMsg2TxCount=0, nGrantUL=1, maxRarWindow=1)),
    ("corner_p3_at2", 3000, dict(maxMsg2TxCount=0, nGrantUL=1, maxRarWindow=1, nPreamble=3, backoff=2, accessTime=2)),
    ("corner_p64_at10", 2000, dict(maxMsg2TxCount=0, nGrantUL=1, maxRarWindow=1, nPreamble=64, backoff=60, accessTime=10)),
    ("corner_p1_65", 65, dict(maxMsg2TxCount=0, nGrantUL=1, maxRarWindow=1, nPreamble=1)),
    ("oracle_msg2_0", 1500, dict(nPreamble=2, backoff=3, nGrantUL=1, maxRarWindow=3, maxMsg2TxCount=0, accessTime=6)),  # ORACLE_CASES' maxMsg2TxCount=0 row
    ("reset_storm", 2600, dict(uniform=1, nPreamble=54, backoff=5, nGrantUL=1, maxRarWindow=1, maxMsg2TxCount=0, accessTime=10)),  # ... and its reset storm
    ("p1_msg2_1", 2000, dict(nPreamble=1, maxMsg2TxCount=1)),
    ("p8_at1", 4000, dict(nPreamble=8, backoff=5, nGrantUL=12, maxRarWindow=2, maxMsg2TxCount=1, accessTime=1)),
    ("p3_b40_at6", 3000, dict(nPreamble=3, backoff=40, nGrantUL=12, maxRarWindow=6, maxMsg2TxCount=3, accessTime=6)),
    ("default_3000", 3000, {}),
    ("default_1", 1, {}), ("default_63", 63, {}), ("default_64", 64, {}), ("default_65", 65, {}),
    ("default_16000", 16000, {}),
]

# Cases that leave a row's kernel by design — a per-subframe capacity of the kernel exceeded, the trial rerun exactly on the next kernel of the
# engine's fallback ladder (prach_engine.hip descend_ladder) — are not counted for that row: the row's kernel never produced their result.  Measured
# on the MI355X with `gpu_kernel_matrix.py --single`; every other case stays on its row's kernel, or the matrix fails.
_NOT_TRIAL_KERNEL = {r["name"] for r in ROWS if r["program"] == "beta" and r["name"] != "legacy_philox"}
LEAVES = {
    # nobody is ever granted: more re-join / reset candidates per subframe than any batch or cluster kernel stages -> trial_kernel only
    "corner_p3_at2": _NOT_TRIAL_KERNEL,
    "reset_storm": _NOT_TRIAL_KERNEL,
    # 4-workgroup lean clusters: a capacity of one workgroup exceeded -> the batch kernel
    "corner_5000": {"lcluster4_philox", "lcluster4_glibc"},
    # fills a calendar list of the 1024-thread batch kernel -> rerun on it with lists of nUE entries (counted as a fallback trial)
    "p3_b40_at6": {"batch_w16_philox", "batch_glibc"},
    # 4032 UE slots per workgroup do not fit LDS next to the Philox lean kernel's tables -> the general cluster kernel (rec_mode 0)
    "default_16000": {"lcluster4_philox"},
    # random case (_random_cases): nPreamble = 1 with Uniform arrivals in the reference's stream -> past the batch kernel's resolver
    "random_42632465": {"batch_glibc"},
}

# NOMA.c cases (nUE, seed, overrides: the engine's names, maxMsg2TxCount = NOMA.c's maxMsg1ReTx), after tests/test_noma.py's NOMA_GPU_CASES
NOMA_CASES = [
    (3000, 0, {}), (64, 3, {}), (1, 4, {}), (5000, 5, dict(nPreamble=8, backoff=3)), (8000, 6, dict(nGrantUL=1, maxMsg2TxCount=3)),
    (6000, 7, dict(nPreamble=64, nGrantUL=5, backoff=40)), (6000, 8, dict(maxRarWindow=6)), (6000, 9, dict(maxRarWindow=7, accessTime=3, nGrantUL=3)),
    (5000, 10, dict(nGrantUL=1, maxMsg2TxCount=0)), (2000, 11, dict(nGrantUL=1, maxMsg2TxCount=0, maxRarWindow=1, nPreamble=2)),
    (10000, 12, {}),
]
RANDOM_CASES = 24  # cases of tests/test_gpu_parity.py's _random_cases added to each batch row's call
