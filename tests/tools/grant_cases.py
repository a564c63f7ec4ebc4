"""The grant sweep: the selection "the Gr lowest-index singleton callers of this subframe get an UL grant" past one wavefront of callers, on every kernel.

Every Beta.c / WithNOMA simulation kernel has an inline copy of that selection (tests/tools/GRANT_SWEEP.md lists them): a one-wavefront form for up to 64
singleton callers and a bin form beyond (counts per index bin of 2^binshift UEs, 1024 bins, a block-wide exclusive prefix, whole bins below the crossing
bin granted, the crossing bin ranked exactly).  The bases of the cut sweep never have more than 17 singleton callers in a subframe.  This module names
base trials that do, classifies every subframe of them FROM THE DEFINITION (sort the indices, take the first Gr: classify() below knows no kernel),
chooses per base the subframes in which each class of the selection occurs, and cuts the trial at t + 1 and t + 2 behind each chosen subframe t: the
grant written in the last subframe is applied by the epilogue (cut t + 1) and by an ordinary pass (cut t + 2).  The rows are cut_cases.CUT_ROWS with the
cluster size each needs at these sizes; the runner is tests/tools/gpu_cut_sweep.py --grant, the comparison the cut sweep's.

Plain data, a generator and CPU-side checks (tests/test_grant_cases_cpu.py): no GPU, no package import.  The generator is deterministic and writes
nothing; every expectation comes from the oracle's grant census (oracle/prach_oracle.c oracle_set_grant_census), never from a GPU run."""
import numpy as np

from oracle import binding as ob
import cut_cases as CC

# ---- the classes --------------------------------------------------------------------------------------------------------------------------------------
# ns: singleton callers of the subframe; Gr = max(0, nGrantUL - 1 - grantCheck) at its head (Beta.c:336-347); bin of a caller: index >> binshift; before(bin):
# callers in lower bins; cnt(bin): callers in it.
CLASSES = ("W64", "W65", "CROSS", "EDGE_LE", "EDGE_GE", "ONE", "ALL", "LAST", "TOP")
#   W64      ns == 64, Gr > 0: the last subframe of the one-wavefront form
#   W65      ns == 65, Gr > 0: the first of the bin form
#   CROSS    ns > 64, 0 < Gr < ns, the crossing bin holds m >= 2 callers of which 0 < j < m are granted: the exact ranking decides
#   EDGE_LE  ns > 64, Gr > 0, a bin with before + cnt == Gr: granted as a whole, by `<=`
#   EDGE_GE  ns > 64, Gr > 0, a caller whose bin has before == Gr: the first one left out, by `>=`
#   ONE      ns > 64, Gr == 1
#   ALL      Gr >= ns > 64: no crossing bin, every caller granted
#   LAST     ns > 64, Gr > 0, a caller in bin 1023: the count and the prefix of the last bin; with before(bin 1023) >= Gr the caller leaves at `before >= Gr`, in
#            front of the `bin + 1 < 1024` arm, so this is NOT a case of that arm
#   TOP      ns > 64, a caller in bin 1023 with before(bin 1023) < Gr: what reaches the `bin + 1 < 1024` arm (a bin at or past the budget leaves in front of it).  FOUND IN NO TRIAL (GRANT_SWEEP.md)
# with sector_grants (WithNOMA:626-637: six budgets, a caller counts against its sector's), key (sector, index >> (binshift + 3)), 128 bins per sector:
SECTOR_CLASSES = ("SECT_CROSS2", "SECT_SPENT", "SECT_W64", "SECT_W65")
#   SECT_CROSS2  ns > 64, two or more sectors each with a crossing bin (0 < j < m granted of its m >= 2 callers)
#   SECT_SPENT   ns > 64, a sector with callers and its budget used up beside a sector with callers and grants left
#   SECT_W64/65  ns == 64 / 65 and a caller's sector has grants left
NBINS = 1024
WAVE = 64


def binshift(nUE):
    """Restated from the engine (layout_launch): the smallest shift with (nUE - 1) >> shift < 1024."""
    s = 0
    while ((nUE - 1) >> s) >= NBINS:
        s += 1
    return s


def definition(idx, left):
    """Who is granted, from the definition: the `left` lowest indices.  Boolean array over idx."""
    idx = np.asarray(idx)
    g = np.zeros(len(idx), dtype=bool)
    g[np.argsort(idx, kind="stable")[:max(0, int(left))]] = True
    return g


def definition_sectors(idx, sector, sleft):
    """The same per sector: of the callers of sector s the sleft[s] lowest indices."""
    g = np.zeros(len(idx), dtype=bool)
    for s in range(6):
        m = np.nonzero(sector == s)[0]
        g[m[definition(idx[m], sleft[s])]] = True
    return g


def _bin_facts(idx, left, shift):
    """(crossing: a bin with before < left < before + cnt, edge_le: a bin with before + cnt == left, edge_ge: a non-empty bin with before == left)."""
    bins, cnt = np.unique(np.asarray(idx) >> shift, return_counts=True)
    before = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    return bool(((before < left) & (left < before + cnt)).any()), bool((before + cnt == left).any()), bool((before == left).any())


def classify(nUE, ns, left, idx, sector=None, sleft=None):
    """The classes of one subframe (a set of names), from the definition alone."""
    out, bs = set(), binshift(nUE)
    if sector is not None:
        have = [s for s in range(6) if (sector == s).any()]
        if ns in (WAVE, WAVE + 1) and any(sleft[s] > 0 for s in have):
            out.add("SECT_W64" if ns == WAVE else "SECT_W65")
        if ns > WAVE:
            if sum(_bin_facts(idx[sector == s], sleft[s], bs + 3)[0] for s in have) >= 2:
                out.add("SECT_CROSS2")
            if any(sleft[s] == 0 for s in have) and any(sleft[s] > 0 for s in have):
                out.add("SECT_SPENT")
        return out
    if left <= 0:
        return out
    if ns == WAVE:
        out.add("W64")
    if ns == WAVE + 1:
        out.add("W65")
    if ns > WAVE:
        cross, le, ge = _bin_facts(idx, left, bs)
        if cross:
            out.add("CROSS")
        if le:
            out.add("EDGE_LE")
        if ge:
            out.add("EDGE_GE")
        if left == 1:
            out.add("ONE")
        if left >= ns:
            out.add("ALL")
        top = int((np.asarray(idx) >> bs == NBINS - 1).sum())
        if top:
            out.add("LAST")
        if top and ns - top < left:  # (before(bin 1023) = ns - cnt(bin 1023): the kernels leave at `before >= Gr` in front of the arm)
            out.add("TOP")
    return out


# ---- the census of a trial (single-threaded: the census hook is process-wide) ---------------------------------------------------------------------------
_census = {}


def census(t):
    """The uncut oracle run of a trial (cut_cases' tuple) with the grant census: dict(res, ues, cen, sub=[(t, ns, left, idx, granted, sector, sleft)])."""
    k = CC.key(t)
    if k not in _census:
        prog, v, n, kw, r, s = t
        assert prog == "beta"
        res, ues, cen = ob.run_trial_grant_census(ob.make_cfg(n, variant=v, **kw), ob.Rng(r, s))
        end = np.concatenate([cen["off"][1:], [len(cen["idx"])]])
        sub = [(int(cen["t"][i]), int(cen["ns"][i]), int(cen["left"][i]), cen["idx"][a:b], cen["granted"][a:b], cen["sector"][a:b], cen["sleft"][i])
               for i, (a, b) in enumerate(zip(cen["off"], end))]
        _census[k] = dict(res=res, ues=ues, cen=cen, sub=sub)
    return _census[k]


def _census_worker(t):
    c = census(t)
    return dict(c, ues=None)


def census_many(trials):
    """census() of several trials at once, in forked child processes (the census hook is process-wide, so threads will not do): fills the cache."""
    import multiprocessing
    import os
    from concurrent.futures import ProcessPoolExecutor
    todo = list({CC.key(t): t for t in trials if CC.key(t) not in _census}.values())
    if len(todo) > 1:
        ob.lib()
        nproc = max(1, min(16, len(todo), int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)))
        with ProcessPoolExecutor(max_workers=nproc, mp_context=multiprocessing.get_context("fork")) as ex:
            for t, c in zip(todo, ex.map(_census_worker, todo)):
                _census[CC.key(t)] = c
    for t in todo:
        census(t)


def classes_of(t):
    """{subframe: set of classes} of the subframes of a trial that are in any class."""
    sect = bool(t[3].get("sector_grants"))
    out = {}
    for tt, ns, left, idx, _, sector, sleft in census(t)["sub"]:
        if ns >= WAVE:
            c = classify(t[2], ns, left, idx, sector if sect else None, sleft if sect else None)
            if c:
                out[tt] = c
    return out


def bin_form(t):
    """The subframes of a trial in which a kernel enters the bin form: ns > 64 with a grant left (with sector_grants: ns > 64)."""
    sect = bool(t[3].get("sector_grants"))
    return [tt for tt, ns, left, *_ in census(t)["sub"] if ns > WAVE and (sect or left > 0)]


def check_definition(t):
    """The oracle's granted set of every subframe of a trial against the sorted-prefix definition.  Returns failure texts."""
    sect = bool(t[3].get("sector_grants"))
    bad = []
    for tt, ns, left, idx, granted, sector, sleft in census(t)["sub"]:
        want = definition_sectors(idx, sector, sleft) if sect else definition(idx, left)
        if len(idx) != ns or not np.array_equal(want, granted):
            bad.append(f"subframe {tt}: ns {ns}, {left} grants left: the oracle granted {idx[granted].tolist()[:8]}.., the definition {idx[want].tolist()[:8]}..")
    return bad


# ---- base trials --------------------------------------------------------------------------------------------------------------------------------------
# (name, nUE, overrides, the classes the base is named for): Beta.c and RandomAccessWithNOMA, seed 700 + variant, each row in its own RNG mode.  All with
# 16 preambles: a subframe has more singleton callers than preambles when buckets emptied by a collision earlier in the scan are called again by UEs
# that re-join in the same subframe (Beta.c:321-330), which takes overload.  Found with the census on the CPU (GRANT_SWEEP.md: the searches).
BASES = [
    # binshift 4, all 1024 bins in use, grants left 5 at most: loaded to the end of the trial, the last 16 UEs (bin 1023) under way from subframe 7191 on (LAST; never inside the budget: no TOP)
    ("g6_16384", 16384, dict(nPreamble=16, nGrantUL=6), ("W64", "W65", "CROSS", "EDGE_LE", "EDGE_GE", "LAST")),
    # one UE past 16 x 1024: binshift 5, bins of 32 UEs, 11 grants
    ("g12_16385", 16385, dict(nPreamble=16, nGrantUL=12), ("CROSS", "EDGE_LE", "EDGE_GE")),
    # nGrantUL = 2: one grant per window, Gr == 1 in every subframe that has one
    ("g2_16000", 16000, dict(nPreamble=16, nGrantUL=2), ("ONE", "CROSS")),
    # 127 grants per window: more than the singleton callers of any subframe (binshift 6)
    ("g128_48000", 48000, dict(nPreamble=16, nGrantUL=128), ("ALL",)),
]
# RandomAccessWithNOMA with the per-sector budgets (PRACH_FLAG_SECTOR_GRANTS): the batch kernel's per-sector form, trial_kernel's per-sector branch
SECTOR_BASES = [
    ("sect_g3_16384", 16384, dict(nPreamble=16, nGrantUL=3, sector_grants=1), ("SECT_CROSS2", "SECT_W64", "SECT_W65")),
]
SEED = 700
PER_CLASS = 2   # chosen subframes per class and trial
MAX_CUTS = 24   # per trial

# ---- rows ---------------------------------------------------------------------------------------------------------------------------------------------
# cut_cases.CUT_ROWS (Beta.c / WithNOMA) with the cluster size each needs at these sizes.  The pins are predicted from choose_kernel (predict_pin below
# restates it, with the LDS figures of kernel_limits.LIMITS); nothing here is copied from a run.
#   lean kernel, Philox: 75 904 + 28 x slots <= 163 840 admits 3 136 owned slots per workgroup: 16 000 UEs on 4 workgroups are 4 032 slots -> 8 workgroups (2 048)
#   lean kernel, rand(): 75 904 + 16 x slots + 8 x groups (rounded up to 64) + 16 x slots / 64 and slots <= 4 096: 16 385 UEs on 4 workgroups are 4 160 slots -> 8
#   general kernel, LDS records: 88 704 + 20 x slots <= 163 840 admits 3 712: 16 000 UEs on 4 workgroups are 4 032 slots -> 8 workgroups
#   48 000 UEs: 16 workgroups (3 008 slots) on every cluster row
LDS_LIMIT, LQCAP = 160 * 1024, 4096
LEAN_TAIL, GENERAL_TAIL_L = 75904, 88704  # (tests/test_grant_cases_cpu.py holds lean_bytes / general_bytes against the library's own size functions)


def lean_bytes(lslots, glibc, groups):
    """lcluster_kernel_lds_bytes restated (prach_lcluster.hip)."""
    if not glibc:
        return LEAN_TAIL + 28 * lslots
    return LEAN_TAIL + 16 * lslots + (groups + 63) // 64 * 64 * 8 + lslots // 64 * 16


def general_bytes(lslots):
    """cluster_kernel_lds_bytes with LDS-resident records restated (prach_cluster.hip)."""
    return GENERAL_TAIL_L + 20 * lslots


ROWS_LEFT_OUT = {}  # (row of cut_cases.CUT_ROWS -> reason: none is left out)
# The compact 8 + 4 byte layout needs a trial the batch kernel cannot take.  The cut sweep arranges that with maxRarWindow = 12, under which no size up to 65 536
# has more than 12 singleton callers in a subframe (the search: GRANT_SWEEP.md); here 65 preambles do it, one past
# batch_max_preambles() (kernel_limits.py: batch_p65_glibc, rec_mode 1), and the bases keep their classes.
FORCE = {"cluster_compact_glibc": dict(nPreamble=65)}
GRANT_ROWS = [dict(r, force=FORCE[r["name"]]) if r["name"] in FORCE else r for r in CC.CUT_ROWS if r["program"] == "beta" and r["name"] not in ROWS_LEFT_OUT]
GROW = {r["name"]: r for r in GRANT_ROWS}
# kernel symbols with a grant selection and the rows that run them (tests/test_grant_cases_cpu.py: every one is run or named in SYMBOLS_LEFT_OUT)
SELECTION_KERNELS = ("batch_kernel<8, false>", "batch_kernel<16, false>", "batch_kernel<16, true>", "lcluster_kernel<false>", "lcluster_kernel<true>",
                     "cluster_kernel<false, 0>", "cluster_kernel<false, 2>", "cluster_kernel<true, 0>", "cluster_kernel<true, 1>", "trial_kernel<false>",
                     "trial_kernel<true>")
SYMBOLS_LEFT_OUT = {}  # (symbol -> reason)
# base trials that leave a row's kernel by a per-subframe capacity (as cut_cases.LEAVES): base name -> {row name: reason}; measured with gpu_cut_sweep.py --grant
LEAVES = {}


def sector_row(row):
    """Rows that take the per-sector bases: trials with the flag go to the batch kernel whatever the cluster option says (run_trials_impl: `sect`), or to
    trial_kernel with legacy = 1."""
    return row["name"].startswith("batch_") or row["name"].startswith("legacy_")


def predict_pin(opts, rng, n, kw):
    """prach_engine.hip run_trials_impl / choose_kernel / batch_eligible / lds_record_slots / use_fast_kernel restated for one launch of trials of n UEs with
    the overrides kw: dict(rec_mode, cluster_size), rec_mode None where the kernel has no record layout (trial_kernel)."""
    o = dict(CC.OPT_DEFAULTS, **opts)
    c = dict(nPreamble=54, backoff=20, maxRarWindow=6, accessTime=5, uniform=0)
    c.update(kw)
    glibc = rng == 0
    if o["legacy"]:
        return dict(rec_mode=None, cluster_size=0)
    need, slots = c["backoff"] + max(c["accessTime"], 5) + c["maxRarWindow"] + 70, 64
    while slots < need:
        slots *= 2
    groups = (n + 63) // 64
    batch_ok = (not o["wide_records"] and c["nPreamble"] <= 64 and c["maxRarWindow"] <= 11 and slots <= 256 and n < (1 << 20) - 1
                and groups <= (2048 if glibc else 1 << 14))
    G = 1 if (c.get("sector_grants") and batch_ok) else o["cluster"]
    assert G >= 1, "these rows all set the cluster size"
    if G == 1 and batch_ok:
        return dict(rec_mode=4, cluster_size=1)
    assert not c.get("sector_grants"), "a per-sector trial outside the batch kernel runs on trial_kernel"
    compact = G == 1 and not o["wide_records"] and glibc and 10000 + c["backoff"] + c["accessTime"] + 64 < 63000
    lslots = (groups + G - 1) // G * 64 if G > 1 and o["lds_records"] else 0
    lean_ok = o["fast"] and o["pipeline"] and c["nPreamble"] <= 64
    if lslots and glibc:
        lslots = lslots if lslots <= LQCAP and lean_ok and groups <= 4096 and lean_bytes(lslots, True, groups) <= LDS_LIMIT else 0
    elif lslots:
        lslots = lslots if lslots <= LQCAP and general_bytes(lslots) <= LDS_LIMIT else 0
    fast = lslots > 0 and (glibc or (lean_ok and lean_bytes(lslots, False, 0) <= LDS_LIMIT))
    return dict(rec_mode=3 if fast else 2 if lslots else 1 if compact else 0, cluster_size=G)


def cluster_for(row, n, kw):
    """The cluster size a row needs for trials of n UEs: its own, or the next power of two up to 32 at which choose_kernel picks the row's kernel."""
    g = row["opts"].get("cluster", 0)
    if g <= 1 or kw.get("sector_grants"):
        return g
    while g <= 32:
        if predict_pin(dict(row["opts"], cluster=g), row["rng"], n, kw)["rec_mode"] == row["pin"]["rec_mode"]:
            return g
        g *= 2
    return None


def sized(row, n, kw):
    """The row as it runs trials of n UEs: the cluster size of cluster_for in its options and its pin (None: no cluster size up to 32 gives the row's kernel)."""
    g = cluster_for(row, n, kw)
    if g is None:
        return None
    if g == row["opts"].get("cluster", 0):
        return row
    return dict(row, opts=dict(row["opts"], cluster=g), pin=dict(row["pin"], cluster_size=g))


def bases_of(row):
    """[(tag, trial, classes named)] of a row: both variants of every base (the per-sector bases: WithNOMA only, the rows of sector_row), with the row's forced
    overrides laid over them; tag is the key of CHOSEN."""
    force = row.get("force", {})
    ftag = "".join(f"_{k}{v}" for k, v in sorted(force.items()))
    out = [(f"{name}_v{v}{ftag}", ("beta", v, n, dict(kw, **force), row["rng"], SEED + v), named) for name, n, kw, named in BASES for v in (0, 1)]
    if sector_row(row):
        out += [(f"{name}_v1{ftag}", ("beta", 1, n, dict(kw, **force), row["rng"], SEED + 1), named) for name, n, kw, named in SECTOR_BASES]
    return [(tag, t, named) for tag, t, named in out if row["name"] not in LEAVES.get(tag.split("_v")[0], {})]


def choose(t, named):
    """The chosen subframes of a trial: per class the base is named for, in the order named, the first subframe of the class and then the first with another
    number of grants left (or else the next one), unless subframes chosen before hold the class PER_CLASS times already.  Sorted."""
    cl = classes_of(t)
    left = {tt: (int(lf) if not t[3].get("sector_grants") else tuple(int(x) for x in sl)) for tt, _, lf, _, _, _, sl in census(t)["sub"]}
    chosen = []
    for c in named:
        cand = [tt for tt in sorted(cl) if c in cl[tt]]
        while sum(c in cl[tt] for tt in chosen) < PER_CLASS:
            have = [tt for tt in chosen if c in cl[tt]]
            rest = [tt for tt in cand if tt not in chosen]
            if not rest:
                break
            other = [tt for tt in rest if all(left[tt] != left[h] for h in have)]
            chosen.append((other or rest)[0])
    return sorted(chosen)


# The chosen subframes per (tag, RNG mode): what choose() yields from the committed oracle, written down so that the GPU runner needs no census run
# (tests/test_grant_cases_cpu.py asserts the table IS what choose() yields; `python tests/tools/grant_cases.py` prints it).
CHOSEN = {
    ('g128_48000_v0', 0): [3301, 3716],
    ('g128_48000_v0', 1): [3351, 3396],
    ('g128_48000_v0_nPreamble65', 0): [3551, 3591],
    ('g128_48000_v1', 0): [3471, 3636],
    ('g128_48000_v1', 1): [3511, 3571],
    ('g128_48000_v1_nPreamble65', 0): [3096, 3551],
    ('g12_16385_v0', 0): [4441, 4566, 4606, 5016],
    ('g12_16385_v0', 1): [4696, 4801, 4846, 4996],
    ('g12_16385_v0_nPreamble65', 0): [5011, 5241, 5491, 5661],
    ('g12_16385_v1', 0): [4531, 4651, 4691, 4891],
    ('g12_16385_v1', 1): [4746, 4786, 5131, 5166],
    ('g12_16385_v1_nPreamble65', 0): [5601, 5656, 5741, 6136],
    ('g2_16000_v0', 0): [3231, 3256, 3766, 3786],
    ('g2_16000_v0', 1): [3101, 3151, 3181, 3396],
    ('g2_16000_v0_nPreamble65', 0): [3226, 3251, 3476, 3856],
    ('g2_16000_v1', 0): [2996, 3016, 3031, 3291],
    ('g2_16000_v1', 1): [2996, 3141, 3566, 3871],
    ('g2_16000_v1_nPreamble65', 0): [3001, 3021, 3426, 4321],
    ('g6_16384_v0', 0): [3891, 3901, 3926, 3976, 4031, 4036, 7216, 7236],
    ('g6_16384_v0', 1): [3471, 3726, 3811, 3891, 3961, 4111, 7191, 7226],
    ('g6_16384_v0_nPreamble65', 0): [3526, 3916, 3996, 4041, 4091, 4121, 7191, 7221],
    ('g6_16384_v1', 0): [3486, 3651, 3666, 3896, 3986, 4126, 7211, 7241],
    ('g6_16384_v1', 1): [3481, 3641, 3691, 3771, 3821, 3881, 7201, 7276],
    ('g6_16384_v1_nPreamble65', 0): [3551, 3571, 3816, 3891, 3996, 4301, 7196, 7201],
    ('sect_g3_16384_v1', 0): [4821, 4956, 5051, 5136, 5141, 5376],
    ('sect_g3_16384_v1', 1): [4696, 4846, 4936, 4946, 5021, 5111],
}


def cuts_of(tag, rng):
    return sorted({c for tt in CHOSEN[(tag, rng)] for c in (tt + 1, tt + 2)})


def trials_of(row):
    """[(row as sized for the trial, tag, base trial, cut, the trial cut there)] of a row."""
    out = []
    for tag, t, _ in bases_of(row):
        srow = sized(row, t[2], t[3])
        assert srow is not None, (row["name"], tag)
        out += [(srow, tag, t, c, CC.with_cut(t, c)) for c in cuts_of(tag, row["rng"])]
    return out


def distinct_bases():
    out = {}
    for row in GRANT_ROWS:
        for tag, t, named in bases_of(row):
            out.setdefault((tag, t[4]), (t, named))
    return out


def coverage(row):
    """{class: chosen subframes of the row's bases in which it occurs} — from the census."""
    cov = {}
    for tag, t, _ in bases_of(row):
        cl = classes_of(t)
        for tt in CHOSEN[(tag, t[4])]:
            for c in cl.get(tt, ()):
                cov[c] = cov.get(c, 0) + 1
    return cov


if __name__ == "__main__":
    census_many([t for t, _ in distinct_bases().values()])
    print("CHOSEN = {")
    for (tag, rng), (t, named) in sorted(distinct_bases().items()):
        print(f"    ({tag!r}, {rng}): {choose(t, named)},")
    print("}")
