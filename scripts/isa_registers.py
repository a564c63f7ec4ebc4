#!/usr/bin/env python3
"""scripts/isa_registers.py [--lib LIB] [KERNEL ...] — register metadata of the kernels in a built library, as the code object's own notes state it:
registers, spills to lanes (scalar) and to scratch (vector), private segment, LDS.  Without a kernel name: both instantiations of the lean kernel.

prach::lcluster_kernel is a chain of short dependent phases (profiles/lcluster_registers.md): a vector register that goes to scratch comes back with a
vector-memory round trip and a full vmcnt(0) on that chain.  tests/test_lcluster_registers.py holds both instantiations to no vector spill and no
private segment.  The notes are read, nothing is disassembled.  CPU only."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "5g-nr-randomaccess_amd")
SHIPPED = os.path.join(PKG, "libprach_hip.so")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
READOBJ = os.path.join(ROCM, "llvm", "bin", "llvm-readobj")
LEAN = ("lcluster_kernel<false>", "lcluster_kernel<true>")
FIELDS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size")

KERNEL = re.compile(r"^  - \.")            # first key of an entry of amdhsa.kernels
KEY = re.compile(r"^(?:    |  - )\.(\w+):\s*(\S.*)?$")  # a key of the entry itself (its arguments' keys are indented further)


def tools_present():
    return os.path.exists(OBJDUMP) and os.path.exists(READOBJ) and shutil.which("c++filt") is not None


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {a: re.sub(r"^void ", "", b.replace("(anonymous namespace)::", "").replace("prach::", "").split("(")[0]) for a, b in zip(names, out)}


def metadata(lib):
    """{kernel: {field: int}} over every gfx950 code object in `lib`."""
    if not os.path.exists(lib):
        raise FileNotFoundError(f"{lib} is not built (make -C 5g-nr-randomaccess_amd/csrc lib)")
    raw = {}
    with tempfile.TemporaryDirectory() as d:
        copy = os.path.join(d, os.path.basename(lib))  # (llvm-objdump --offloading writes LIB.N.<triple> next to its input)
        shutil.copyfile(lib, copy)
        subprocess.run([OBJDUMP, "--offloading", copy], capture_output=True, text=True, check=True, cwd=d)
        objs = sorted(f for f in os.listdir(d) if f.endswith("gfx950"))
        if not objs:
            raise RuntimeError(f"no gfx950 code object in {lib}")
        for f in objs:
            notes = subprocess.run([READOBJ, "--notes", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in notes.split("\n"):
                if line.startswith("amdhsa.") and not line.startswith("amdhsa.kernels"):
                    cur = None
                if KERNEL.match(line):
                    cur = {}
                m = KEY.match(line)
                if m and cur is not None:
                    cur[m.group(1)] = (m.group(2) or "").strip()
                    if m.group(1) == "name":
                        raw[cur["name"]] = cur
    names = demangle(sorted(raw))
    return {names[k]: {f: int(v[f]) for f in FIELDS if f in v} for k, v in raw.items()}


def table(meta, kernels):
    rows = ["| kernel | " + " | ".join(f"`.{f}`" for f in FIELDS) + " |", "|---|" + "---|" * len(FIELDS)]
    for k in kernels:
        rows.append(f"| `{k}` | " + " | ".join(str(meta[k].get(f, "?")) for f in FIELDS) + " |")
    return "\n".join(rows)


def main(argv):
    lib = SHIPPED
    if "--lib" in argv:
        at = argv.index("--lib")
        lib = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
    meta = metadata(lib)
    kernels = argv or list(LEAN)
    missing = [k for k in kernels if k not in meta]
    if missing:
        print(f"not in {lib}: {missing}; it has {sorted(meta)}", file=sys.stderr)
        return 1
    print(table(meta, kernels))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
