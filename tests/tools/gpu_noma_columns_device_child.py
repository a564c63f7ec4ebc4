"""Child process of tests/test_gpu_noma_census.py: the DEVICE destination of the NOMA columns (Engine.run_trials_noma_columns(device=True),
prach_run_trials_noma_columns_device).  torch is imported BEFORE the package loads its library, so both share one HIP runtime.  Prints `ok ...` and exits
0, or raises."""
import ctypes as C
import os
import sys

import torch  # noqa: F401  (first: the one HIP runtime of this process is torch's)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
FIELDS = ["state", "arrival", "lost", "raw:timer", "sector", "sojourn"]
SENTINEL = 0x1234567


def main():
    cfgs = [pkg.make_cfg(2000, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=6, nGrantUL=1, maxMsg2TxCount=3, max_steps=4325),
            pkg.make_cfg(8193, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=2, max_steps=3000),
            pkg.make_cfg(65, variant=pkg.VARIANT_NOMA_C, rng_mode=pkg.RNG_PHILOX, seed=3)]
    eng = pkg.Engine(0)
    n, rows = len(cfgs), sum(c.nUE for c in cfgs)
    res_h, _, host = eng.run_trials_noma_columns(cfgs, FIELDS)
    assert len(pkg.hip_runtimes()) == 1, pkg.hip_runtimes()
    res_d, _, dev = eng.run_trials_noma_columns(cfgs, FIELDS, device=True)
    assert isinstance(dev.data, torch.Tensor) and dev.data.is_cuda and dev.data.dtype == torch.int32 and tuple(dev.data.shape) == host.data.shape == (len(FIELDS), rows)
    assert np.array_equal(dev.data.cpu().numpy(), host.data) and [bytes(a) for a in res_d] == [bytes(b) for b in res_h]
    assert all(np.array_equal(dev.headers[f], host.headers[f]) for f in host.headers.dtype.names) and dev.fields == host.fields
    tm = eng.timing()
    assert tm.noma_columns_ms > 0 and (tm.noma_census_ms, tm.columns_ms, tm.pick_ms, tm.xtab_ms, tm.trace_ms, tm.summary_ms, tm.dist_ms, tm.timeline_ms, tm.sojourn_ms) == (0,) * 9

    # a torch reduction on the tensor: the bincount of the STATE column is the census's state marginal
    _, _, cs = eng.run_trials_noma_census(cfgs, ("one", 1, 1), ("state", 1, 9), groups=[0] * n)
    counts = torch.bincount(dev.column("state"), minlength=9).cpu().numpy()
    assert counts.tolist() == cs.cells[0, 0, :9].tolist() and int(counts.sum()) == rows and int(cs.cells[0, 0, 9]) == 0 and not cs.cells[0, 1].any()
    assert counts[:8].all()  # (the all-states trial is among them)

    # the C entry point on a tensor with rows behind the sum of nUE: they keep the sentinel, in every column
    L = pkg.lib()
    arr = (pkg.PrachCfg * n)(*cfgs)
    res = (pkg.PrachResult * n)()
    hdr = (pkg.PrachNomaColumns * n)()
    sp, ids = pkg.noma_columns_spec(FIELDS)
    cap = rows + 5
    t = torch.full((len(ids), cap), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert L.prach_run_trials_noma_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, t.data_ptr(), cap) == 0
    got = t.cpu().numpy()
    assert np.array_equal(got[:, :rows], host.data) and (got[:, rows:] == SENTINEL).all()
    assert [h.offset for h in hdr] == host.offsets.tolist() and [h.idle + h.served + h.dropped + h.pending for h in hdr] == [c.nUE for c in cfgs]

    # refusals: a NULL destination, host memory, a capacity one short, a misaligned pointer, the reference's stream — before the fill and before any launch
    t.fill_(SENTINEL)
    torch.cuda.synchronize()
    before = bytes(hdr)
    host_mem = np.full((len(ids), cap), SENTINEL, dtype=np.int32)
    assert L.prach_run_trials_noma_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, None, cap) == -1
    assert L.prach_run_trials_noma_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, host_mem.ctypes.data, cap) == -1
    assert L.prach_run_trials_noma_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, t.data_ptr(), rows - 1) == -1
    assert L.prach_run_trials_noma_columns_device(eng._h, arr, n, res, None, C.byref(sp), hdr, t.data_ptr() + 2, cap) == -1
    glibc = (pkg.PrachCfg * n)(*cfgs)
    glibc[1].rng_mode = pkg.RNG_GLIBC
    assert L.prach_run_trials_noma_columns_device(eng._h, glibc, n, res, None, C.byref(sp), hdr, t.data_ptr(), cap) == -2
    torch.cuda.synchronize()
    assert bool((t == SENTINEL).all()) and (host_mem == SENTINEL).all() and bytes(hdr) == before
    eng.close()
    print("ok device destination")


main()
