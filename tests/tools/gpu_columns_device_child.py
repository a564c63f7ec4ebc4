"""Child process of tests/test_gpu_columns.py: the DEVICE destination of the per-UE columns (Engine.run_trials_columns(device=True),
prach_run_trials_columns_device).  torch is imported BEFORE the package loads its library, so both share one HIP runtime; under the argument `reversed` the
library is loaded first and the binding must refuse.  Prints `ok ...` and exits 0, or raises."""
import ctypes as C
import os
import sys

MODE = sys.argv[1] if len(sys.argv) > 1 else "torch_first"
if MODE == "torch_first":
    import torch  # noqa: F401  (first: the one HIP runtime of this process is torch's)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
FIELDS = ["arrival", "sojourn", "state", "raw:timer", "age", "sojourn"]
SENTINEL = 0x1234567


def cfgs_of():
    return [pkg.make_cfg(3000, variant=0, rng_mode=pkg.RNG_PHILOX, seed=1), pkg.make_cfg(2000, variant=1, rng_mode=pkg.RNG_PHILOX, seed=2, maxMsg2TxCount=3),
            pkg.make_cfg(300, variant=0, rng_mode=pkg.RNG_PHILOX, seed=4, max_steps=3), pkg.make_cfg(8193, variant=0, rng_mode=pkg.RNG_GLIBC, seed=5),
            pkg.make_cfg(65, variant=1, rng_mode=pkg.RNG_GLIBC, seed=6)]


def main():
    cfgs = cfgs_of()
    if MODE == "reversed":
        pkg.lib()  # the library, and with it the system's HIP runtime, before torch
        eng = pkg.Engine(0)
        try:
            eng.run_trials_columns(cfgs, FIELDS, device=True)
        except pkg.PrachError as e:
            assert e.status == -1 and "before torch" in str(e), str(e)
            res, _, col = eng.run_trials_columns(cfgs, FIELDS)  # ... and the host destination goes on
            assert all(r.status == 0 for r in res) and col.data.shape == (len(FIELDS), sum(c.nUE for c in cfgs))
            print("ok refused: " + str(e)[:60])
            return
        raise AssertionError("device=True after the library was loaded first: not refused")

    import torch
    eng = pkg.Engine(0)
    n, rows = len(cfgs), sum(c.nUE for c in cfgs)
    res_h, _, host = eng.run_trials_columns(cfgs, FIELDS)
    assert len(pkg.hip_runtimes()) == 1, pkg.hip_runtimes()
    res_d, _, dev = eng.run_trials_columns(cfgs, FIELDS, device=True)
    assert isinstance(dev.data, torch.Tensor) and dev.data.is_cuda and dev.data.dtype == torch.int32 and tuple(dev.data.shape) == host.data.shape == (len(FIELDS), rows)
    assert np.array_equal(dev.data.cpu().numpy(), host.data) and [bytes(a) for a in res_d] == [bytes(b) for b in res_h]
    assert all(np.array_equal(dev.headers[f], host.headers[f]) for f in host.headers.dtype.names) and dev.fields == host.fields
    assert np.array_equal(dev.trial(3).cpu().numpy(), host.trial(3)) and np.array_equal(dev.column("state").cpu().numpy(), host.column("state"))
    tm = eng.timing()
    assert tm.columns_ms > 0 and (tm.pick_ms, tm.xtab_ms, tm.trace_ms, tm.summary_ms, tm.dist_ms, tm.timeline_ms, tm.sojourn_ms) == (0,) * 7

    # the C entry point on a tensor with rows behind the sum of nUE: they keep the sentinel, in every column
    L = pkg.lib()
    arr = (pkg.PrachCfg * n)(*cfgs)
    res = (pkg.PrachResult * n)()
    hdr = (pkg.PrachColumns * n)()
    sp, ids = pkg.columns_spec(FIELDS)
    cap = rows + 5
    t = torch.full((len(ids), cap), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.prach_run_trials_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, t.data_ptr(), cap) == 0
    got = t.cpu().numpy()
    assert np.array_equal(got[:, :rows], host.data) and (got[:, rows:] == SENTINEL).all()
    assert [h.offset for h in hdr] == host.offsets.tolist() and [h.idle + h.served + h.unserved for h in hdr] == [c.nUE for c in cfgs]

    # refusals: a NULL destination, host memory (a numpy array's address), a capacity one short — before the fill and before any launch: the tensor is untouched
    t.fill_(SENTINEL)
    torch.cuda.synchronize()
    before = bytes(hdr)
    host_mem = np.full((len(ids), cap), SENTINEL, dtype=np.int32)
    assert L.prach_run_trials_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, None, cap) == -1
    assert L.prach_run_trials_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, host_mem.ctypes.data, cap) == -1
    assert L.prach_run_trials_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, t.data_ptr(), rows - 1) == -1
    assert L.prach_run_trials_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, t.data_ptr() + 2, cap) == -1  # (not a multiple of 4 bytes)
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all()) and (host_mem == SENTINEL).all() and bytes(hdr) == before

    # a torch reduction on the tensor: the sum of the sojourn over the served UEs of every trial is the summary's sojourn_sum
    _, _, sm = eng.run_trials_summary(cfgs)
    soj, state = dev.column("sojourn").to(torch.int64), dev.column("state")
    for k, c in enumerate(cfgs):
        o = int(dev.offsets[k])
        s = slice(o, o + c.nUE)
        assert int(soj[s][state[s] == 1].sum()) == int(sm.rows["sojourn_sum"][k]) and int((state[s] == 1).sum()) == int(sm.rows["success"][k]) == int(dev.headers["served"][k])
    assert int(sm.rows["sojourn_sum"].sum()) > 0
    eng.close()
    print("ok device destination")


main()
