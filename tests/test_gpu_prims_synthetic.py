"""The device building blocks every trial kernel is made of, on inputs no trial produces: tests/tools/gpu_prims_harness.hip runs philox_draw31 / _x2,
pass_masks<false | true> / light_case, wave_scan_incl / wave_sum / wave_max, fastmod / slot_align in every form, sector_of_draw, mk_granule / granule_ok,
cluster_block and hot_encode / hot_decode / hot_fits / slot_of / idx_of on the cases of tests/tools/prims_cases.py — one child process per section and
build (the product's flags, and the NOBITOP3 flags of csrc/Makefile): sixteen on the device, one at a time, plus one `--host` run of the mask section
that never opens the device.  Every section's output is identical under the two builds and equals a plain reference: the pinned oracle's Philox, numpy in
int64, Python integer arithmetic, and for the masks the branched per-UE body.  tests/test_prims_cases_cpu.py holds the cases and references without a GPU."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import harness as H  # noqa: E402
import prims_cases as P  # noqa: E402

pytestmark = pytest.mark.gpu

latch = H.Latch()  # a harness run that ended abnormally (exit status, signal, timeout): no later test of this file starts another one


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return P.build_harness(tmp_path_factory.mktemp("prims_harness"))


@pytest.fixture(scope="module")
def consts(harness):
    return P.harness_constants(harness["product"])


def _both_builds(harness, section, n, payload, d, **kw):
    """The section under both builds, one child each; the two outputs must be identical.  Returns the words (int64)."""
    case = str(d / "case.bin")
    P.write_case(case, section, n, payload, **kw)
    out = {}
    for build in P.BUILDS:
        res = str(d / f"result_{build}.bin")
        with latch.child(f"{section} ({build})"):
            P.run_harness(harness[build], section, case, res, timeout=120)
        out[build] = P.read_result(res, section, 0, n)
    assert out["product"].shape == out["nobitop3"].shape and (out["product"] == out["nobitop3"]).all(), \
        f"{section}: the two builds differ in {(out['product'] != out['nobitop3']).sum()} words, first at {np.flatnonzero(out['product'] != out['nobitop3'])[:5]}"
    return out["product"].astype(np.int64), case


def _first(bad, names=None):
    k = np.flatnonzero(bad)[:6]
    return f"{int(np.asarray(bad).sum())} cases, first {[names[i] for i in k] if names is not None else k.tolist()}"


# ---- 1 philox ----
def test_philox_draws_equal_the_oracle(ob, harness, tmp_path):
    cases = P.philox_cases()
    got, _ = _both_builds(harness, "philox", len(cases), [cases], tmp_path)
    got = got.reshape(-1, 4)
    ref = P.philox_reference(ob, cases)
    assert got[:3, 0].tolist() == [exp[0] >> 1 for _, _, exp in P.PHILOX_KAT]  # the Random123 vectors, on the device
    for col, what in enumerate(("philox_draw31", "philox_draw31_x2, first draw", "philox_draw31_x2, second draw (c1 + 1 mod 2^32, no carry)")):
        bad = got[:, col] != ref[:, col]
        assert not bad.any(), f"{what}: {_first(bad)}: {[hex(v) for v in cases[np.flatnonzero(bad)[0]]]}"


# ---- 2 masks ----
@pytest.fixture(scope="module")
def masks(harness, consts, tmp_path_factory):
    M = P.mask_cases(consts)
    d = tmp_path_factory.mktemp("masks")
    case = str(d / "case.bin")
    P.write_masks(case, M)
    bits = None
    for build in P.BUILDS:
        res = str(d / f"result_{build}.bin")
        with latch.child(f"masks ({build})"):
            P.run_harness(harness[build], "masks", case, res, timeout=120)
        b = P.read_result(res, "masks", 0, M.n)
        assert bits is None or (bits == b).all(), f"masks: the two builds differ, first at {np.flatnonzero(bits != b)[:5]}"
        bits = b
    host = str(d / "host.bin")
    P.run_harness(harness["product"], "masks", case, host, host=True, timeout=300)  # the branched body on the CPU: no device
    T = P.MaskTable(M, P.read_result(host, "masks", 1, M.n), consts)
    bits = bits.astype(np.int64)
    assert (bits >> 9 == 0).all()
    B = {name: ((bits >> k) & 1).astype(bool) for k, name in enumerate(("light", "quiet", "done", "trig", "light_spec", "quiet_spec", "done_spec", "trig_spec", "light_case"))}
    front = np.repeat(M.groups[:, 2] == 1, 64)
    enumerated = M.recs[:, 0] == 0
    return M, T, B, front, enumerated


def test_masks_without_a_front(masks):
    M, T, B, front, enumerated = masks
    k = ~front & enumerated
    assert k.sum() > 1_000_000
    for s in ("", "_spec"):
        assert not (k & (B["trig" + s] != T.trig)).any(), "trig " + s + _first(k & (B["trig" + s] != T.trig))
        assert not (k & (B["done" + s] != T.done)).any(), "done " + s + _first(k & (B["done" + s] != T.done))
        bad = k & B["quiet" + s] & ~T.noop
        assert not bad.any(), f"quiet{s} lanes on which the body does something: {_first(bad)}"
        bad = k & B["light" + s] & ~T.light_state
        assert not bad.any(), f"light{s} lanes the body does not leave in the light path's state: {_first(bad)}"
        assert not (k & B["light" + s] & B["quiet" + s]).any()
    bad = k & (B["light"] != T.pred)
    assert not bad.any(), f"pass_masks<false>.light against the predicate: {_first(bad)}"
    bad = k & (B["light_spec"] != T.pred_spec)
    assert not bad.any(), f"pass_masks<true>.light against the predicate without PEND_CALLER: {_first(bad)}"
    bad = k & (B["light_case"] != T.pred)
    assert not bad.any(), f"light_case against the predicate: {_first(bad)}"
    n = k.sum()  # the classes are all there, in every wavefront's mix
    assert (k & B["light"]).sum() >= 0.01 * n and (k & B["quiet"]).sum() >= 0.01 * n and (k & ~B["light"] & ~B["quiet"]).sum() >= 0.01 * n
    assert (k & T.pred & ~T.pred_spec).sum() > 1000


def test_masks_in_the_arrival_front(masks):
    M, T, B, front, enumerated = masks
    fg = np.flatnonzero(M.groups[:, 2] == 1)
    assert len(fg) == 210
    lane = np.arange(64)
    for g in fg:
        t, _, _, i0, acNow, acPrev, nUE, _ = M.groups[g].tolist()
        s, tw = slice(64 * g, 64 * g + 64), slice(64 * M.twin[g], 64 * M.twin[g] + 64)
        i = i0 + lane
        old, new, gone = i < acPrev, (i >= acPrev) & (i < acNow), i >= acNow
        for sfx in ("", "_spec"):
            light, quiet, done, trig = (B[n + sfx][s] for n in ("light", "quiet", "done", "trig"))
            where = f"group {g} (acPrev, acNow, nUE at lanes {acPrev - i0}, {acNow - i0}, {nUE - i0}){sfx}"
            assert (light[old] == B["light" + sfx][tw][old]).all() and (quiet[old] == B["quiet" + sfx][tw][old]).all(), where + ": lanes below acPrev"
            assert not light[new].any() and not quiet[new].any(), where + ": a lane that must be activated"
            assert quiet[gone].all() and not light[gone].any(), where + ": lanes past acNow"
            assert (done == (((i < acNow) & T.done[s]) | (i >= nUE))).all(), where + ": done"
            assert (trig == T.trig[s]).all(), where + ": trig"
        assert (B["light_case"][s] == B["light_case"][tw]).all()
    # the twins (the same records without a front) hold light and quiet lanes where the front forbids them
    tw = np.zeros(M.n, dtype=bool)
    for g in fg:
        tw[64 * M.twin[g]:64 * M.twin[g] + 64] = True
    assert (tw & B["light"]).sum() > 500 and (tw & B["quiet"]).sum() > 500
    k = tw & enumerated  # and are themselves held to the body
    assert not (k & B["quiet"] & ~T.noop).any() and not (k & B["light"] & ~T.light_state).any() and not (k & (B["light"] != T.pred)).any()


# ---- 3 wave ----
def test_wave_scan_sum_max_equal_numpy(harness, tmp_path):
    cases = P.wave_cases()
    names = [n for n, _ in cases]
    rows = np.stack([r for _, r in cases]).astype(np.int64)
    got, _ = _both_builds(harness, "wave", len(rows), [rows], tmp_path)
    got = got.reshape(len(rows), 64, 4)
    scan, total, top = P.wave_reference(rows)
    bad = (got[:, :, 0] != scan).any(axis=1)
    assert not bad.any(), f"wave_scan_incl: {_first(bad, names)}: lanes {np.flatnonzero(got[np.flatnonzero(bad)[0], :, 0] != scan[np.flatnonzero(bad)[0]])[:8]}"
    bad = (got[:, :, 1] != total[:, None]).any(axis=1)  # every lane holds the sum
    assert not bad.any(), f"wave_sum: {_first(bad, names)}"
    bad = (got[:, :, 2] != top[:, None]).any(axis=1)    # every lane holds the maximum
    assert not bad.any(), f"wave_max: {_first(bad, names)}"


# ---- 4 mod ----
def test_fastmod_and_slot_align_equal_python_on_the_device(harness, tmp_path):
    cases = P.mod_cases()
    got, case = _both_builds(harness, "mod", len(cases), [cases], tmp_path)
    got = got.reshape(-1, 8)
    mod, sa = P.mod_reference(cases)
    for col, what, ref in ((0, "fastmod", mod), (1, "fastmod_flat", mod), (2, "slot_align_fm", sa), (3, "slot_align_flat", sa), (4, "slot_align", sa)):
        bad = got[:, col] != ref
        assert not bad.any(), f"{what}: {_first(bad)}: (x, d, sub, aT) = {cases[np.flatnonzero(bad)[0]].tolist()}"
    host = str(tmp_path / "host.bin")
    P.run_harness(harness["product"], "mod", case, host, host=True)
    assert (P.read_result(host, "mod", 1, len(cases)).astype(np.int64).reshape(-1, 8) == got).all()  # host and device forms agree everywhere


# ---- 5 sector ----
def test_sector_of_draw_equals_the_float32_statement(harness, tmp_path):
    d = P.sector_cases()
    got, _ = _both_builds(harness, "sector", len(d), [d], tmp_path)
    bad = got != P.sector_reference(d)
    assert not bad.any(), f"sector_of_draw: {_first(bad)}: draws {d[np.flatnonzero(bad)[:6]].tolist()}"


# ---- 6 granule ----
def test_granule_tag_and_values(harness, consts, tmp_path):
    g = P.granule_cases(consts)
    got, _ = _both_builds(harness, "granule", len(g), [g], tmp_path)
    got = got.reshape(-1, 4)
    w0, w1, ok, probe = P.granule_reference(g)
    made = g[:, 0] == 0
    assert ok[made].all() and not probe.any() and not ok[~made].any()
    for col, what, ref in ((0, "low word", w0), (1, "high word", w1), (2, "granule_ok under its own tag", ok), (3, "granule_ok under another tag", probe)):
        bad = got[:, col] != ref
        assert not bad.any(), f"{what}: {_first(bad)}: (kind, lo, hi, tag, probe) = {[hex(v) for v in g[np.flatnonzero(bad)[0]]]}"
    # the two 20-bit values come back exactly, and nothing of a 32-bit input reaches the tag bits or bits 24..31 of the high word
    assert ((got[made, 0] & 0xFFFFF) == (g[made, 1] & 0xFFFFF)).all() and ((got[made, 1] & 0xFFFFF) == (g[made, 2] & 0xFFFFF)).all() and (got[made, 1] >> 24 == 0).all()


# ---- 7 blocks ----
def test_cluster_block_is_a_bijection(harness, tmp_path):
    sets = P.block_sets()
    got, _ = _both_builds(harness, "blocks", len(sets), [sets], tmp_path)
    at = 0
    for G, xpack, ntrials, grid in sets.tolist():
        w = got[at:at + 64 * grid].reshape(grid, 64)
        at += 64 * grid
        where = f"G {G} xpack {xpack} ntrials {ntrials}"
        assert (w == w[:, :1]).all(), where + ": lanes of a block disagree"
        w = w[:, 0]
        ok, fits, T, b = (w >> 31) & 1 == 1, (w >> 30) & 1 == 1, (w >> 8) & 0xFFFFF, w & 0xFF
        assert fits[ok].all() and (T[ok] < ntrials).all() and (b[ok] < G).all(), where + ": a block past the last trial returns true, or b >= G"
        key = T[ok] * G + b[ok]
        assert len(key) == ntrials * G and (np.sort(key) == np.arange(ntrials * G)).all(), where + ": not onto {0..ntrials-1} x {0..G-1} exactly once each"
        assert not ok[fits & (T >= ntrials)].any(), where
        if xpack:
            bx = np.arange(grid)[ok]
            for trial in np.unique(T[ok]):
                assert len(set((bx[T[ok] == trial] % 8).tolist())) == 1, where + f": trial {trial} spans several blockIdx.x % 8"
    assert at == len(got)


# ---- 8 hot ----
def test_hot_record_and_slot_helpers(harness, consts, tmp_path):
    h = P.hot_cases(consts)
    pairs = P.slot_pairs(consts)
    lslots = consts["CLUSTER_LQCAP"]  # the largest lslots the engine uses
    got, _ = _both_builds(harness, "hot", len(h), [h[:, :3], pairs], tmp_path, p3=len(pairs), p4=lslots)
    a, s = got[:8 * len(h)].reshape(-1, 8), got[8 * len(h):].reshape(len(pairs), lslots, 2)
    fits = h[:, 3] == 1
    bad = a[:, 6] != h[:, 3]
    assert not bad.any(), f"hot_fits: {_first(bad)}: (tx, bo) = {h[np.flatnonzero(bad)[0], :2].tolist()}"
    for col, what, ref in ((2, "txTime", h[:, 0]), (3, "nowBackoff", h[:, 1]), (4, "packed word", h[:, 2]), (0, "packed word as stored", h[:, 2])):
        bad = fits & (P.as_i32(a[:, col]) != P.as_i32(ref))
        assert not bad.any(), f"hot_decode(hot_encode): {what}: {_first(bad)}: (tx, bo, pk) = {h[np.flatnonzero(bad)[0], :3].tolist()}"
    assert (a[:, 5] == 0x7b7b7b7b).all()  # the timer base is the caller's
    B = consts["HOT_BO_BIAS"]
    assert (a[fits, 1] == (((h[fits, 0] + 1) & 0xFFFF) | ((h[fits, 1] + B) << 16))).all()  # the biased 16-bit packing itself
    idx = P.idx_of_reference(pairs, lslots)
    bad = (s[:, :, 0] != idx).any(axis=1)
    assert not bad.any(), f"idx_of: {_first(bad)}: (G, b) = {pairs[np.flatnonzero(bad)[0]].tolist()}"
    bad = (s[:, :, 1] != np.arange(lslots)[None, :]).any(axis=1)
    assert not bad.any(), f"slot_of(idx_of(slot)): {_first(bad)}: (G, b) = {pairs[np.flatnonzero(bad)[0]].tolist()}"
