"""The limit table: every hard limit the engine's kernel choice rests on, with a case on its last value inside and its first outside.

prach_engine.hip picks one of six kernels per launch (choose_kernel, batch_eligible, lds_record_slots, use_fast_kernel, the solo / small routing
of run_trials_impl).  Each choice rests on a limit of the kernel it picks, restated by hand in the engine, in the kernel's own guard and in the
packed records.  tests/tools/gpu_kernel_limits.py runs every case below on the GPU against the oracle (bit-exact, full bar) and compares the
call's prach_timing with the pin the ENGINE'S SOURCE predicts for that side; tests/test_kernel_limits.py proves without a GPU, from the oracle
alone, that every case stands where this table says, and that every limit function of prach_device.h has an entry.  Plain data: no GPU, no
oracle, no package import.  The engine (prach_engine.hip) is cited by function name; line numbers are given for the kernel files and the host C."""

# ---- the limits -------------------------------------------------------------------------------------------------------------------------------
# name -> where it is stated, which exported limit functions / constants of prach_device.h it covers, last value inside, first outside
LIMITS = {
    "batch_preambles": dict(
        source=["prach_engine.hip batch_eligible", "prach_batch.hip:70 NPB", "prach_batch.hip:241 guard", "prach_batch.hip:1017"],
        covers=["batch_max_preambles"], inside=64, outside=65, what="nPreamble, cluster=1"),
    "lcluster_preambles": dict(
        source=["prach_engine.hip lds_record_slots / use_fast_kernel", "prach_lcluster.hip:53 NPCL", "prach_lcluster.hip:348 guard", "prach_lcluster.hip:969"],
        covers=["lcluster_max_preambles"], inside=64, outside=65, what="nPreamble, cluster=4 and 16"),
    "noma_preambles": dict(
        source=["prach_engine.hip run_trials_impl"], covers=[], inside=64, outside=65, what="nPreamble of NOMA.c: 65 is PRACH_ERR_UNSUPPORTED"),
    "batch_rar_window": dict(
        source=["prach_engine.hip batch_eligible", "prach_batch.hip:241 guard (literal 11)", "prach_batch.hip:1018,1021"],
        covers=["batch_max_rar_window", "batch_max_rar_window_two_per_cu"], inside=11, outside=12,
        what="maxRarWindow, cluster=1.  The engine asks batch_max_rar_window() for both workgroup shapes; batch_max_rar_window_two_per_cu() has no caller and the same "
             "value: the 512-thread shape (batch_waves=8) has a pair of its own all the same"),
    "calendar_128_256": dict(
        source=["prach_batch.hip:1023 batch_calendar_slots", "prach_engine.hip layout_launch (slots and chunk pool)", "prach_batch.hip:242 guard"],
        covers=["batch_calendar_slots"], inside=128, outside=129, what="need = backoff + max(accessTime, 5) + maxRarWindow + 70: 128 slots / 256 slots, both the batch kernel"),
    "calendar_256_leave": dict(
        source=["prach_engine.hip batch_eligible", "prach_batch.hip:73 CR", "prach_batch.hip:241 guard", "prach_batch.hip:1029"],
        covers=["batch_max_calendar_slots"], inside=256, outside=257, what="the same need: 256 slots / no batch kernel"),
    "compact_record": dict(
        source=["prach_engine.hip choose_kernel", "prach_cluster.hip:264 hot_fits"],
        covers=[], inside=2935, outside=2936, what="backoff + accessTime with Uniform arrivals (60 000 + backoff + accessTime + 64 < 63 000), glibc, cluster=1, batch kernel ineligible"),
    "subframe_16bit": dict(
        source=["prach_cluster.hip:261 hot record (16-bit txTime + 1)", "prach_lcluster.hip:348 / prach_cluster.hip:747 guards (stop >= 0xFFFE: the 16-bit granule tags)",
                "prach_engine.hip batch_eligible and choose_kernel keep the 16-bit forms away"],
        covers=[], inside=65535, outside=65536, what="largest txTime of the trial (the oracle's log): every route must carry it in 32 bits"),
    "glibc_batch_groups": dict(
        source=["prach_engine.hip batch_eligible", "prach_batch.hip:131 BGG", "prach_batch.hip:241 guard", "prach_batch.hip:1020"],
        covers=["batch_max_groups"], inside=131072, outside=131073, what="nUE in the reference's stream, cluster=1 (Philox: 2^14 groups = 2^20 UEs, behind the 20-bit limit: never deciding)"),
    "glibc_cluster_size": dict(
        source=["prach_engine.hip run_trials_impl", "prach_device.h:152 CLUSTER_GLIBC_MAX_UE", "prach_cluster.hip:96 GSCAP", "prach_cluster.hip:747 guard", "prach_lcluster.hip:968"],
        covers=["CLUSTER_GLIBC_MAX_UE", "lcluster_max_groups_glibc"], inside=262144, outside=262145,
        what="nUE in the reference's stream on any cluster kernel.  lcluster_max_groups_glibc() = 4096 groups is the same size and never decides on its own: "
             "4096 groups in lslots <= CLUSTER_LQCAP need 64 workgroups, whose layout (175 232 bytes) is past CLUSTER_LDS_LIMIT"),
    "lds_slots_philox": dict(
        source=["prach_engine.hip lds_record_slots / use_fast_kernel", "prach_lcluster.hip:964 lcluster_kernel_lds_bytes", "prach_cluster.hip:1209 cluster_kernel_lds_bytes"],
        covers=["lcluster_kernel_lds_bytes"], inside=3136, outside=3200,
        what="owned UE slots per workgroup, Philox, lean kernel: the LDS-BYTE test binds, not CLUSTER_LQCAP — 75 904 + 28 x slots <= 163 840 admits 3 136 slots "
             "(rec_mode 3); beyond, the records stay in LDS on the general kernel (rec_mode 2)"),
    "lds_slots_general": dict(
        source=["prach_engine.hip lds_record_slots", "prach_cluster.hip:1209 cluster_kernel_lds_bytes"],
        covers=["cluster_kernel_lds_bytes"], inside=3712, outside=3776,
        what="owned UE slots per workgroup, Philox, the general kernel's LDS-resident layout: bytes again — 88 704 + 20 x slots <= 163 840 admits 3 712 slots "
             "(rec_mode 2), beyond: global records (rec_mode 0)"),
    "lds_slots_glibc": dict(
        source=["prach_engine.hip lds_record_slots", "prach_device.h:132 CLUSTER_LQCAP", "prach_lcluster.hip:65,348", "prach_cluster.hip:148,747"],
        covers=["CLUSTER_LQCAP"], inside=4096, outside=4160,
        what="owned UE slots per workgroup, the reference's stream (16 bytes per slot): CLUSTER_LQCAP binds with 16 and with 32 workgroups — 4 096 slots take 150 656 bytes "
             "in a 16-workgroup cluster (1 024 groups) and 158 848 in a 32-workgroup one (2 048 groups); 4 160 slots would still fit the bytes (152 720 / 160 400)"),
    "ue_index_20bit": dict(
        source=["prach_engine.hip batch_eligible", "prach_engine.hip NOMA.c `small`", "prach_engine.hip `solo`", "prach_batch.hip:241 guard (nUE >= 1 << 20)", "GR_NONE = 0xFFFFF and & 0xFFFFF in the cluster kernels"],
        covers=[], inside=1048574, outside=1048575, what="nUE: 20-bit UE index inside an exchange granule, 0xFFFFF reserved"),
    "largest_size": dict(
        source=["prach_host.c:55 prach_cfg_validate"], covers=[], inside=1 << 24, outside=(1 << 24) + 1, what="nUE: 2^24 + 1 is PRACH_ERR_UNSUPPORTED"),
}

# The clause `maxTime + backoff + accessTime + 128 < 65000` of batch_eligible (batch_max_subframes()) decides for no valid configuration: the
# calendar clause next to it needs backoff + max(accessTime, 5) + maxRarWindow + 70 <= 256, so backoff + accessTime <= 185, and maxTime is 60 000 at most
# (prach_host.c:64): 60 000 + 185 + 128 = 60 313 < 65 000 always.  It is covered from the far side only (subframe_16bit: backoff 6000 leaves the batch kernel,
# by the calendar clause first).
UNREACHABLE = {"batch_subframes_clause": dict(covers=["batch_max_subframes"], why="batch_eligible: implied by the calendar clause (backoff + accessTime <= 185, maxTime <= 60 000)")}

OPT_DEFAULTS = dict(cluster=0, batch_waves=0, wide_records=0, legacy=0)  # (every option a case sets, at the engine's defaults)
PHILOX, GLIBC = 1, 0
BETA, WITHNOMA, NOMA = 0, 1, 2

CASES = []


def _case(limit, side, name, variant, nUE, kw, rng, opts, pin, expect="exact", pre=None, seed=11):
    """side: "in" / "out" of the limit.  pin: the prach_timing fields the engine's source predicts (fallback_trials == 0 and trial_kernel_reruns == 0 are added
    to every pin).  expect: "exact" (bit-exact against the oracle) or "unsupported" (the call returns PRACH_ERR_UNSUPPORTED).  pre: what the oracle alone must
    show about the case (tests/test_kernel_limits.py)."""
    assert limit in LIMITS and side in ("in", "out")
    CASES.append(dict(limit=limit, side=side, name=name, variant=variant, nUE=nUE, kw=dict(kw), rng=rng, seed=seed, opts=dict(opts),
                      pin=dict(pin, fallback_trials=0, trial_kernel_reruns=0) if expect == "exact" else {}, expect=expect, pre=dict(pre or {})))


def _need(kw):
    c = dict(backoff=20, accessTime=5, maxRarWindow=6)
    c.update(kw)
    return c["backoff"] + max(c["accessTime"], 5) + c["maxRarWindow"] + 70


_RN = {PHILOX: "philox", GLIBC: "glibc"}
# What runs one workgroup per trial when the batch kernel cannot (choose_kernel): the general cluster kernel with 16-byte records (rec_mode 0); in the
# reference's stream with the compact 8 + 4 byte records (rec_mode 1) while every subframe number fits 16 bits (Beta arrivals: 10 000 subframes).
_NOT_BATCH = {PHILOX: dict(rec_mode=0, cluster_size=1), GLIBC: dict(rec_mode=1, cluster_size=1)}
_BATCH = dict(rec_mode=4, cluster_size=1)

# ---- nPreamble ----
for _r in (PHILOX, GLIBC):
    _case("batch_preambles", "in", f"batch_p64_{_RN[_r]}", BETA, 3000, dict(nPreamble=64), _r, dict(cluster=1), _BATCH)           # measured: rec_mode 4
    _case("batch_preambles", "out", f"batch_p65_{_RN[_r]}", BETA, 3000, dict(nPreamble=65), _r, dict(cluster=1), _NOT_BATCH[_r])  # measured: 0 / 1
    for _g in (4, 16):
        # 65 preambles: Philox keeps the records in LDS on the general kernel (rec_mode 2: lds_record_slots admits them, use_fast_kernel does not);
        # in the reference's stream only the lean kernel has LDS records (rec_mode 0)
        _case("lcluster_preambles", "in", f"lcluster{_g}_p64_{_RN[_r]}", WITHNOMA, 6000, dict(nPreamble=64, nGrantUL=54), _r, dict(cluster=_g), dict(rec_mode=3, cluster_size=_g))
        _case("lcluster_preambles", "out", f"lcluster{_g}_p65_{_RN[_r]}", WITHNOMA, 6000, dict(nPreamble=65, nGrantUL=54), _r, dict(cluster=_g),
              dict(rec_mode=2 if _r == PHILOX else 0, cluster_size=_g))
_case("noma_preambles", "in", "noma_p64", NOMA, 6000, dict(nPreamble=64, nGrantUL=5), PHILOX, dict(cluster=4), dict(cluster_size=4))
_case("noma_preambles", "out", "noma_p65", NOMA, 6000, dict(nPreamble=65, nGrantUL=5), PHILOX, dict(cluster=4), {}, expect="unsupported")
_case("noma_preambles", "out", "noma_p65_glibc", NOMA, 2000, dict(nPreamble=65), GLIBC, {}, {}, expect="unsupported")

# ---- maxRarWindow ----
for _r in (PHILOX, GLIBC):
    _case("batch_rar_window", "in", f"batch_rar11_{_RN[_r]}", WITHNOMA, 3000, dict(maxRarWindow=11, nGrantUL=54), _r, dict(cluster=1), _BATCH)
    _case("batch_rar_window", "out", f"batch_rar12_{_RN[_r]}", WITHNOMA, 3000, dict(maxRarWindow=12, nGrantUL=54), _r, dict(cluster=1), _NOT_BATCH[_r])
# (the 512-thread shape of the batch kernel: the same limit)
_case("batch_rar_window", "in", "batch_rar11_w8", WITHNOMA, 3000, dict(maxRarWindow=11, nGrantUL=54), PHILOX, dict(cluster=1, batch_waves=8), _BATCH)
_case("batch_rar_window", "out", "batch_rar12_w8", WITHNOMA, 3000, dict(maxRarWindow=12, nGrantUL=54), PHILOX, dict(cluster=1, batch_waves=8), _NOT_BATCH[PHILOX])

# ---- the batch kernel's calendar: need = backoff + max(accessTime, 5) + maxRarWindow + 70 ----
for _r in (PHILOX, GLIBC):
    _case("calendar_128_256", "in", f"cal128_{_RN[_r]}", BETA, 20000, dict(backoff=47), _r, dict(cluster=1), _BATCH, pre=dict(need=128))
    _case("calendar_128_256", "out", f"cal129_{_RN[_r]}", BETA, 20000, dict(backoff=48), _r, dict(cluster=1), _BATCH, pre=dict(need=129))
    _case("calendar_256_leave", "in", f"cal256_{_RN[_r]}", BETA, 20000, dict(backoff=175), _r, dict(cluster=1), _BATCH, pre=dict(need=256))
    _case("calendar_256_leave", "out", f"cal257_{_RN[_r]}", BETA, 20000, dict(backoff=176), _r, dict(cluster=1), _NOT_BATCH[_r], pre=dict(need=257))
# accessTime > 5, so that max(accessTime, 5) decides: backoff 39 + 13 + 6 + 70 = 128
_case("calendar_128_256", "in", "cal128_at13", WITHNOMA, 8000, dict(backoff=39, accessTime=13, nGrantUL=54), PHILOX, dict(cluster=1), _BATCH, pre=dict(need=128))
_case("calendar_128_256", "out", "cal129_at13", WITHNOMA, 8000, dict(backoff=40, accessTime=13, nGrantUL=54), PHILOX, dict(cluster=1), _BATCH, pre=dict(need=129))
# 256 slots under load (every UE cycles through backoff: 12 000 UEs on 3 grants).  layout_launch sizes the chunk pool for 128 open chunks per wavefront whatever
# the slot count; these cases run without a fallback trial on that pool (measured), on either side of 128: txTime is aligned to the access slots, so only
# every fifth subframe ahead receives records and a wavefront has some 40 open chunks, not 256.  That argument does not hold for accessTime < 5: a loaded
# 256-slot trial with accessTime = 1 is NOT in this table and has not been run.
_LOADED = dict(nGrantUL=3, maxRarWindow=6)
_case("calendar_128_256", "in", "cal128_loaded", WITHNOMA, 12000, dict(_LOADED, backoff=47), PHILOX, dict(cluster=1), _BATCH, pre=dict(need=128))
_case("calendar_128_256", "out", "cal129_loaded", WITHNOMA, 12000, dict(_LOADED, backoff=48), PHILOX, dict(cluster=1), _BATCH, pre=dict(need=129))
_case("calendar_256_leave", "in", "cal256_loaded", WITHNOMA, 12000, dict(_LOADED, backoff=175), PHILOX, dict(cluster=1), _BATCH, pre=dict(need=256))
_case("calendar_256_leave", "in", "cal256_loaded_glibc", WITHNOMA, 12000, dict(_LOADED, backoff=175), GLIBC, dict(cluster=1), _BATCH, pre=dict(need=256))

# ---- 16-bit subframe numbers: Uniform arrivals over 60 000 subframes, overloaded (14 000 UEs on one grant per 5 subframes) so that UEs are still
#      under way at subframe 60 000; maxRarWindow = 12 keeps the batch kernel away ----
_UNI = dict(uniform=1, nGrantUL=2, maxRarWindow=12)
_case("compact_record", "in", "compact_2935", BETA, 14000, dict(_UNI, backoff=2930), GLIBC, dict(cluster=1), dict(rec_mode=1, cluster_size=1), pre=dict(uniform_runs_out=1, tx_below=65536))
_case("compact_record", "out", "compact_2936", BETA, 14000, dict(_UNI, backoff=2931), GLIBC, dict(cluster=1), dict(rec_mode=0, cluster_size=1), pre=dict(uniform_runs_out=1, tx_below=65536))
# backoff 6000: the oracle's largest txTime is past 65 535.  Every route, and the record form that ran: one workgroup per trial on 16-byte records
# (Philox: the batch kernel is out by its calendar, glibc: not compact); 4 workgroups — 3 520 slots each — Philox LDS records on the general kernel,
# glibc on the lean one; 16 workgroups on the lean kernel; trial_kernel.
_TX = dict(uniform=1, nGrantUL=2, backoff=6000)
_PRE_TX = dict(uniform_runs_out=1, tx_at_least=65536)
_case("subframe_16bit", "in", "tx16_in_lean16_philox", BETA, 14000, dict(uniform=1, nGrantUL=2, backoff=4806), PHILOX, dict(cluster=16), dict(rec_mode=3, cluster_size=16),
      pre=dict(uniform_runs_out=1, tx_below=65536))
for _r in (PHILOX, GLIBC):
    _case("subframe_16bit", "out", f"tx16_wg1_{_RN[_r]}", BETA, 14000, _TX, _r, dict(cluster=1), dict(rec_mode=0, cluster_size=1), pre=_PRE_TX)
    _case("subframe_16bit", "out", f"tx16_wg4_{_RN[_r]}", BETA, 14000, _TX, _r, dict(cluster=4), dict(rec_mode=2 if _r == PHILOX else 3, cluster_size=4), pre=_PRE_TX)
    _case("subframe_16bit", "out", f"tx16_wg16_{_RN[_r]}", BETA, 14000, _TX, _r, dict(cluster=16), dict(rec_mode=3, cluster_size=16), pre=_PRE_TX)
    _case("subframe_16bit", "out", f"tx16_legacy_{_RN[_r]}", BETA, 14000, _TX, _r, dict(legacy=1), dict(cluster_size=0), pre=_PRE_TX)

# ---- sizes in the reference's stream ----
_BIG = dict(large=1)
_case("glibc_batch_groups", "in", "bgg_131072", WITHNOMA, 131072, dict(nGrantUL=54, max_steps=3000), GLIBC, dict(cluster=1), _BATCH, pre=_BIG)
_case("glibc_batch_groups", "out", "bgg_131073", WITHNOMA, 131073, dict(nGrantUL=54, max_steps=3000), GLIBC, dict(cluster=1), _NOT_BATCH[GLIBC], pre=_BIG)
# 262 144 UEs: automatic = 32 workgroups (cluster_size: the cap), 8 192 / 16 384 slots each are past CLUSTER_LQCAP: global records (rec_mode 0)
_case("glibc_cluster_size", "in", "gmax_262144_auto", BETA, 262144, dict(max_steps=2000), GLIBC, {}, dict(rec_mode=0, cluster_size=32), pre=_BIG)
_case("glibc_cluster_size", "out", "gmax_262145_auto", BETA, 262145, dict(max_steps=2000), GLIBC, {}, dict(cluster_size=0), pre=_BIG)
_case("glibc_cluster_size", "in", "gmax_262144_wg16", BETA, 262144, dict(max_steps=2000), GLIBC, dict(cluster=16), dict(rec_mode=0, cluster_size=16), pre=_BIG)
_case("glibc_cluster_size", "out", "gmax_262145_wg16", BETA, 262145, dict(max_steps=2000), GLIBC, dict(cluster=16), dict(cluster_size=0), pre=_BIG)

# ---- LDS-resident slots: nUE = slots x workgroups is the largest size admitted, + 64 UEs is one more group = 64 more slots ----
for _g in (16, 32):
    _case("lds_slots_philox", "in", f"lslots3136_wg{_g}", BETA, 3136 * _g, dict(max_steps=4000), PHILOX, dict(cluster=_g), dict(rec_mode=3, cluster_size=_g), pre=_BIG)
    _case("lds_slots_philox", "out", f"lslots3200_wg{_g}", BETA, 3136 * _g + 64, dict(max_steps=4000), PHILOX, dict(cluster=_g), dict(rec_mode=2, cluster_size=_g), pre=_BIG)
_case("lds_slots_general", "in", "lslots3712_wg16", BETA, 3712 * 16, dict(max_steps=4000), PHILOX, dict(cluster=16), dict(rec_mode=2, cluster_size=16), pre=_BIG)
_case("lds_slots_general", "out", "lslots3776_wg16", BETA, 3712 * 16 + 64, dict(max_steps=4000), PHILOX, dict(cluster=16), dict(rec_mode=0, cluster_size=16), pre=_BIG)
_case("lds_slots_glibc", "in", "lslots4096_wg16_glibc", BETA, 4096 * 16, dict(max_steps=4000), GLIBC, dict(cluster=16), dict(rec_mode=3, cluster_size=16), pre=_BIG)
_case("lds_slots_glibc", "out", "lslots4160_wg16_glibc", BETA, 4096 * 16 + 64, dict(max_steps=4000), GLIBC, dict(cluster=16), dict(rec_mode=0, cluster_size=16), pre=_BIG)
_case("lds_slots_glibc", "in", "lslots4096_wg32_glibc", BETA, 4096 * 32, dict(max_steps=2000), GLIBC, dict(cluster=32), dict(rec_mode=3, cluster_size=32), pre=_BIG)
_case("lds_slots_glibc", "out", "lslots4160_wg32_glibc", BETA, 4096 * 32 + 64, dict(max_steps=2000), GLIBC, dict(cluster=32), dict(rec_mode=0, cluster_size=32), pre=_BIG)

# ---- the 20-bit UE index.  UEs arrive in index order (Beta.c:121-134), so only a trial that runs most of its 10 000 subframes puts UEs with an index past
#      2^20 under way: the sizes past the limit run long (trial_kernel has no capacity to exceed), the last size inside runs short, on light load ----
_case("ue_index_20bit", "in", "ue1048574_auto", BETA, 1048574, dict(max_steps=400), PHILOX, {}, dict(rec_mode=0, cluster_size=32), pre=_BIG)
_case("ue_index_20bit", "in", "ue1048574_batch", WITHNOMA, 1048574, dict(max_steps=400), PHILOX, dict(cluster=1), _BATCH, pre=_BIG)
_case("ue_index_20bit", "out", "ue1048575_auto", BETA, 1048575, dict(max_steps=4000), PHILOX, {}, dict(cluster_size=0), pre=_BIG)
_case("ue_index_20bit", "out", "ue1048575_wg1", WITHNOMA, 1048575, dict(max_steps=2000), PHILOX, dict(cluster=1), dict(cluster_size=0), pre=_BIG)
_case("ue_index_20bit", "out", "ue1048576_auto", WITHNOMA, 1048576, dict(max_steps=2000), PHILOX, {}, dict(cluster_size=0), pre=_BIG)
_case("ue_index_20bit", "out", "ue1100000_long", BETA, 1100000, dict(max_steps=8000), PHILOX, {}, dict(cluster_size=0), pre=dict(large=1, index_past=1 << 20))
# the reference's stream: past CLUSTER_GLIBC_MAX_UE already, trial_kernel on both sides
_case("ue_index_20bit", "in", "ue1048574_glibc", WITHNOMA, 1048574, dict(max_steps=1000), GLIBC, {}, dict(cluster_size=0), pre=_BIG)
_case("ue_index_20bit", "out", "ue1048575_glibc", WITHNOMA, 1048575, dict(max_steps=1000), GLIBC, {}, dict(cluster_size=0), pre=_BIG)
_case("ue_index_20bit", "out", "ue1100000_glibc", BETA, 1100000, dict(max_steps=3500), GLIBC, {}, dict(cluster_size=0), pre=_BIG)
# NOMA.c, Philox: 16 workgroups inside (cluster_size with the cap 16), one workgroup outside (`small` in run_trials_impl)
_case("ue_index_20bit", "in", "noma1048574", NOMA, 1048574, dict(max_steps=400), PHILOX, {}, dict(cluster_size=16), pre=_BIG)
_case("ue_index_20bit", "out", "noma1048575", NOMA, 1048575, dict(max_steps=3000), PHILOX, {}, dict(cluster_size=1), pre=_BIG)
# The last size inside, long enough that UE indices past 2^19 travel in the 20-bit fields of the cluster / NOMA exchange granules (by subframe 4500 more than half
# of the UEs have arrived): heavily overloaded, so a per-subframe capacity may hand the trial on (LEAVES) — exact on whichever kernel.
_case("ue_index_20bit", "in", "ue1048574_long", BETA, 1048574, dict(max_steps=4500), PHILOX, {}, dict(rec_mode=0, cluster_size=32), pre=dict(large=1, index_past=1 << 19))
_case("ue_index_20bit", "in", "noma1048574_long", NOMA, 1048574, dict(max_steps=4500), PHILOX, {}, dict(cluster_size=16), pre=dict(large=1, index_past=1 << 19))
# NOMA.c in the reference's stream: run_noma_glibc hands every size to the single-launch form (noma_glibc_launch), which has no `small` / `solo` test in
# front of it and no granule fields (one workgroup per trial): the same route on both sides, no cluster launch (cluster_size 0), one launch
_case("ue_index_20bit", "in", "noma1048574_glibc", NOMA, 1048574, dict(max_steps=400), GLIBC, {}, dict(cluster_size=0, launches=1), pre=_BIG)
_case("ue_index_20bit", "out", "noma1048575_glibc", NOMA, 1048575, dict(max_steps=400), GLIBC, {}, dict(cluster_size=0, launches=1), pre=_BIG)

# ---- the largest accepted size: max_steps = 150 keeps the oracle's call at 2^24 UEs under the slowest other case of this table (7.7 s against
#      85 s for ue1100000_long; ue1048574_long takes 19.5 s and noma1048574_long 11.3 s — one core each, measured side by side) ----
_case("largest_size", "in", "ue2p24", BETA, 1 << 24, dict(max_steps=150), PHILOX, {}, dict(cluster_size=0), pre=_BIG)
_case("largest_size", "out", "ue2p24_plus1", BETA, (1 << 24) + 1, dict(max_steps=150), PHILOX, {}, {}, expect="unsupported")

# One call that mixes a trial past the 20-bit limit with ordinary ones (run_trials_impl: `solo` / `rest`): the ordinary ones in one launch of their own (three small trials: the batch
# kernel, one workgroup each — rec_mode 4 stays in prach_timing), the large one on trial_kernel afterwards (the call's last launch: cluster_size 0), every trial exact.
MIXED_CALL = dict(name="mixed_solo_rest", limit="ue_index_20bit", rng=PHILOX, opts={}, pin=dict(cluster_size=0, launches=2, fallback_trials=0, trial_kernel_reruns=0),
                  trials=[(BETA, 20000, {}, 21), (BETA, 1048575, dict(max_steps=1000), 22), (WITHNOMA, 30000, {}, 23), (BETA, 3000, {}, 24)])

# Cases that leave their pinned kernel by a per-subframe capacity (as kernel_matrix.LEAVES): name -> reason.  At most one case in eight, never the
# only case of a side.
LEAVES = {
    "ue1048574_long": "half a million UEs under way on 54 grants: a per-subframe capacity of a cluster workgroup may be exceeded, the ladder reruns the trial exactly",
    "noma1048574_long": "the same load on noma_kernel's mailboxes: rerun with one workgroup per trial (a fallback trial)",
}

# Measured on the MI355X (tests/tools/gpu_kernel_limits.py, 72 cases 0 bad, 112 s of which the oracle's calls take 83 s on 8 threads): the prach_timing every
# case reported — each equals the pin its entry expects.  The cases added after that run (the 512-thread pair, 32-workgroup glibc clusters, the long and the
# NOMA.c reference-stream cases at the 20-bit limit) have no measured pin on file yet.  (rec_mode of a call that ends on trial_kernel or runs noma_kernel is the engine's initial 0 or
# the previous launch's: those kernels have no record layout, their pins name cluster_size only.)
MEASURED = {
    "batch_p64_philox": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "batch_p65_philox": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster4_p64_philox": "rec_mode=3 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster4_p65_philox": "rec_mode=2 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster16_p64_philox": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster16_p65_philox": "rec_mode=2 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "batch_p64_glibc": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "batch_p65_glibc": "rec_mode=1 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster4_p64_glibc": "rec_mode=3 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster4_p65_glibc": "rec_mode=0 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster16_p64_glibc": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lcluster16_p65_glibc": "rec_mode=0 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "noma_p64": "rec_mode=0 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "noma_p65": "PRACH_ERR_UNSUPPORTED",
    "noma_p65_glibc": "PRACH_ERR_UNSUPPORTED",
    "batch_rar11_philox": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "batch_rar12_philox": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "batch_rar11_glibc": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "batch_rar12_glibc": "rec_mode=1 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal128_philox": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal129_philox": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal256_philox": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal257_philox": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal128_glibc": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal129_glibc": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal256_glibc": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal257_glibc": "rec_mode=1 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal128_at13": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal129_at13": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal128_loaded": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal129_loaded": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal256_loaded": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "cal256_loaded_glibc": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "compact_2935": "rec_mode=1 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "compact_2936": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_in_lean16_philox": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_wg1_philox": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_wg4_philox": "rec_mode=2 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_wg16_philox": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_legacy_philox": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_wg1_glibc": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_wg4_glibc": "rec_mode=3 cluster_size=4 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_wg16_glibc": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "tx16_legacy_glibc": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "bgg_131072": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "bgg_131073": "rec_mode=1 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "gmax_262144_auto": "rec_mode=0 cluster_size=32 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "gmax_262145_auto": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "gmax_262144_wg16": "rec_mode=0 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "gmax_262145_wg16": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots3136_wg16": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots3200_wg16": "rec_mode=2 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots3136_wg32": "rec_mode=3 cluster_size=32 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots3200_wg32": "rec_mode=2 cluster_size=32 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots3712_wg16": "rec_mode=2 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots3776_wg16": "rec_mode=0 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots4096_wg16_glibc": "rec_mode=3 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "lslots4160_wg16_glibc": "rec_mode=0 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048574_auto": "rec_mode=0 cluster_size=32 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048574_batch": "rec_mode=4 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048575_auto": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048575_wg1": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048576_auto": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1100000_long": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048574_glibc": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1048575_glibc": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue1100000_glibc": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "noma1048574": "rec_mode=0 cluster_size=16 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "noma1048575": "rec_mode=0 cluster_size=1 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue2p24": "rec_mode=0 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=1",
    "ue2p24_plus1": "PRACH_ERR_UNSUPPORTED",
    "mixed_solo_rest": "rec_mode=4 cluster_size=0 fallback_trials=0 trial_kernel_reruns=0 launches=2",
}
