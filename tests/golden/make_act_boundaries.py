"""Writes tests/golden/act_boundaries.json: (angle draw, radius draw) pairs at cellRadius 100 whose r cos(angle), r sin(angle) or sqrt(1 + env^2) — the three
doubles the reference's activeUE rounds to float (NOMA.c:176-178,186) — lie next to a float rounding boundary under the C library's libm:

  must   |dropped 29 bits - 2^28| <= ACT_BAND / 2: the device's near_float_boundary must fire (it would not only if the device's own value were more than
         ACT_BAND / 2 double ulps off the host's);
  near   the same distance in [4 ACT_BAND, 8 ACT_BAND]: it must not.

Each case is about ONE of the three quantities: the other two are at least 4 ACT_BAND away from every boundary, so a check that forgets one term fails on
that term's cases.  The must-flag cases of a quantity lie on both sides of the midpoint.  numpy's cos / sin only prefilter; membership is decided with the
C library's (stream_act_cases.Host.quantities).  Run once on a CPU (a few minutes):  python tests/golden/make_act_boundaries.py
tests/test_stream_act_cases_cpu.py re-classifies the file under the libm of the machine it runs on."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import stream_act_cases as S  # noqa: E402

ACT_BAND = 64  # csrc/prach_noma_act.h (tests/test_stream_act_cases_cpu.py holds the file's value against the compiled one)
RADIUS = 100.0
MUST, NEAR = 12, 8
PER_SIDE = dict(px=4, py=4, pld=0)  # (1 + env^2 is a float plus a rounding error: its root meets a boundary at few values only, mostly from one side)
BATCH, MAX_BATCHES = 4_000_000, 400
QS = ("px", "py", "pld")


def main():
    import __graft_entry__ as g
    H = S.Host(g.load_package())
    rng = np.random.default_rng(20221128)
    have = {(q, kind): [] for q in QS for kind in ("must", "near")}

    def full(q):
        m = have[(q, "must")]
        return len(m) >= MUST and sum(c["side"] > 0 for c in m) >= PER_SIDE[q] and sum(c["side"] < 0 for c in m) >= PER_SIDE[q] and len(have[(q, "near")]) >= NEAR

    for batch in range(MAX_BATCHES):
        if all(full(q) for q in QS):
            break
        ad = rng.integers(0, 2**31, size=BATCH, dtype=np.int64)
        rd = rng.integers(int(0.13 * 2**31), 2**31, size=BATCH, dtype=np.int64)  # r = 100 sqrt(u) > 36
        px, py, pld, _ = S.quantities_np(ad, rd, RADIUS)
        d = np.stack([S.boundary_distance(v) for v in (px, py, pld)])
        cand = np.flatnonzero(((d <= ACT_BAND // 2 + 16) | ((d >= 4 * ACT_BAND - 16) & (d <= 8 * ACT_BAND + 16))).any(axis=0))
        for i in cand:
            vals = H.quantities(int(ad[i]), int(rd[i]), RADIUS)
            if not vals[3] > 35.0:
                continue
            dist = [int(S.boundary_distance(v)) for v in vals[:3]]
            for k, q in enumerate(QS):
                others = [dist[j] for j in range(3) if j != k]
                if min(others) < 4 * ACT_BAND:
                    continue
                bits = int(np.float64(vals[k]).view(np.int64)) & ((1 << 29) - 1)
                c = dict(q=q, angle=int(ad[i]), rdraw=int(rd[i]), dist=dist[k], side=1 if bits >= 1 << 28 else -1)
                if q != "pld" and any(x["value"] == vals[k].hex() for kind in ("must", "near") for x in have[(q, kind)]):
                    continue  # (the same double again; sqrt(1 + env^2) has only a handful of such values at this radius, reached from many x, y)
                c["value"] = vals[k].hex()
                if dist[k] <= ACT_BAND // 2:
                    m = have[(q, "must")]
                    if len(m) < MUST or sum(x["side"] == c["side"] for x in m) < PER_SIDE[q]:
                        m.append(dict(c, kind="must"))
                elif 4 * ACT_BAND <= dist[k] <= 8 * ACT_BAND and len(have[(q, "near")]) < NEAR:
                    have[(q, "near")].append(dict(c, kind="near"))
        print(f"batch {batch}: " + ", ".join(f"{q} {len(have[(q, 'must')])} / {len(have[(q, 'near')])}" for q in QS), flush=True)
    assert all(full(q) for q in QS), "not enough cases found"
    cases = [c for q in QS for kind in ("must", "near") for c in have[(q, kind)]]
    with open(S.BOUNDARIES_JSON, "w") as f:
        json.dump(dict(radius=RADIUS, act_band=ACT_BAND, pairs_searched=(batch) * BATCH, cases=cases), f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases after {batch * BATCH} pairs")


if __name__ == "__main__":
    main()
