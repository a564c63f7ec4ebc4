"""The registers of prach::lcluster_kernel, from the built libraries' own metadata (CPU only: scripts/isa_registers.py reads the code object's notes).

The kernel's subframe is a chain of short dependent phases; a vector register sent to scratch comes back with a vector-memory round trip behind a full
vmcnt(0) on that chain (profiles/lcluster_registers.md: two loop-invariant LDS addresses did, in round 2 of every subframe).  Both instantiations are
held to no vector spill and no private segment, in the shipped library and in the two variant builds the GPU suite runs (the small-queue test build and
the one without v_bitop3; the diagnostic build may spill, as its header comment says).  Metadata only: no instruction is searched for.  A library that
is not built, or missing LLVM tools, skip."""
import importlib.util
import os

import pytest

from conftest import ROOT

LIBS = ["libprach_hip.so", "libprach_hip_tinyq.so", "libprach_hip_nobitop3.so"]
KERNELS = ["lcluster_kernel<false>", "lcluster_kernel<true>"]


def _isa():
    spec = importlib.util.spec_from_file_location("isa_registers", os.path.join(ROOT, "scripts", "isa_registers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_meta = {}


def metadata_of(lib):
    isa = _isa()
    path = os.path.join(isa.PKG, lib)
    if not isa.tools_present():
        pytest.skip("llvm-objdump / llvm-readobj / c++filt not found")
    if not os.path.exists(path):
        pytest.skip(f"{path} is not built")
    if lib not in _meta:
        _meta[lib] = isa.metadata(path)
        print(lib)
        print(isa.table(_meta[lib], KERNELS))
    return _meta[lib]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("lib", LIBS)
def test_lean_kernel_spills_no_vector_register(lib, kernel):
    meta = metadata_of(lib)
    assert kernel in meta, sorted(meta)
    k = meta[kernel]
    print(lib, kernel, k)
    assert k["vgpr_spill_count"] == 0, k
    assert k["private_segment_fixed_size"] == 0, k
    assert 0 < k["vgpr_count"] <= 128, k  # (1024 threads per workgroup: four wavefronts per SIMD)
