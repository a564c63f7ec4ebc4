"""The compiler-chosen boolean instructions of the shipped kernels, on file (CPU only: the gfx950 code objects are disassembled here).

ROCm 7.2 folded the batched kernel's mask algebra into a v_bitop3_b32 with a wrong truth table once (LABNOTES, round 4).  The cross-check is
libprach_hip_nobitop3.so, the same library built without the instruction, run against the oracle next to the shipped one on every kernel that has
such a table (tests/tools/gpu_kernel_matrix.py, from tests/test_gpu_parity.py).  Here, without a GPU: the cross-check build really has none of
them, the shipped library's tables are the ones on file (tests/golden/bitop3_inventory.json, scripts/isa_bitop3.py), and every kernel with a
table the compiler chose is pinned by a row of the GPU matrix (tests/tools/kernel_matrix.py)."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

PKG_DIR = os.path.join(ROOT, "5g-nr-randomaccess_amd")
REGEN = "compiler-chosen boolean instructions changed: run the GPU cross-check (`pytest -m gpu -k bitop3`), then `scripts/isa_bitop3.py --write`"


def _isa():
    spec = importlib.util.spec_from_file_location("isa_bitop3", os.path.join(ROOT, "scripts", "isa_bitop3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa():
    """Both libraries built first (the Makefile's dependencies: nothing to do when they are fresh, so neither can be stale)."""
    csrc = os.path.join(PKG_DIR, "csrc")
    subprocess.check_call(["make", "-C", csrc, "lib", "ARCH=gfx950"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "lib", "NOBITOP3=1", "ARCH=gfx950"], stdout=subprocess.DEVNULL)
    return _isa()


@pytest.fixture(scope="module")
def shipped(isa):
    return isa.inventory(isa.SHIPPED)


def test_cross_check_build_has_no_bitop3(isa):
    """(a) the cross-check build differs from the shipped one in exactly this instruction: not one v_bitop3 site in any kernel."""
    inv = isa.inventory(isa.NOBITOP3)
    assert len(inv) >= 10, f"too few kernels found in {isa.NOBITOP3}: {sorted(inv)}"
    left = {k: t for k, t in inv.items() if t}
    assert not left, (f"libprach_hip_nobitop3.so still contains v_bitop3 (does `make NOBITOP3=1` still pass "
                      f"-Xclang -target-feature -Xclang -bitop3-insts?): {left}")


def test_shipped_inventory_is_on_file(isa, shipped):
    """(b) every kernel's truth tables and site counts as recorded: a kernel edit or a compiler update that moves one is seen here."""
    with open(isa.GOLDEN) as f:
        golden = json.load(f)
    d = isa.diff(golden["kernels"], shipped)
    assert not d, REGEN + f"\n  (on file: {golden['compiler']}, here: {isa.compiler_version()})\n  " + "\n  ".join(d)


def test_every_chosen_table_is_cross_checked(isa, shipped):
    """(c) every kernel with a table other than the Philox xor3 (0x96) is pinned by a row of the GPU matrix, and every kernel a row names exists."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    try:
        from kernel_matrix import COVERAGE
    finally:
        sys.path.pop(0)
    with open(isa.GOLDEN) as f:
        golden = json.load(f)["kernels"]
    need = set(isa.kernels_with_chosen_tables(shipped)) | set(isa.kernels_with_chosen_tables(golden))
    missing = sorted(need - set(COVERAGE))
    assert not missing, f"kernels with compiler-chosen v_bitop3 tables that no row of tests/tools/kernel_matrix.py pins: {missing}"
    unknown = sorted(set(COVERAGE) - set(shipped))
    assert not unknown, f"tests/tools/kernel_matrix.py names kernels the library does not have: {unknown}"
