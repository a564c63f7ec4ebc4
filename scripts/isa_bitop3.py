#!/usr/bin/env python3
"""scripts/isa_bitop3.py [--lib LIB] [--write | --check] — inventory of gfx950's three-input boolean instruction (v_bitop3_b16 / v_bitop3_b32) in a
built library: per kernel, the number of sites of each truth table.  Without an option it prints the table.

ROCm 7.2 folded the batched kernel's mask algebra into a v_bitop3_b32 with a wrong truth table once (LABNOTES, round 4).  Every table the compiler
chooses is therefore on file (tests/golden/bitop3_inventory.json) and every kernel that has one is cross-checked on the GPU against the oracle, with
the shipped library and with the one built without the instruction (tests/tools/gpu_kernel_matrix.py).  A kernel edit or a compiler update that moves
a table changes the inventory, and tests/test_isa_bitop3.py says so.
  --write   regenerate tests/golden/bitop3_inventory.json from the shipped library
  --check   compare the shipped library with it (exit status 1 and the difference on a mismatch)
CPU only: the code objects are taken out of the library and disassembled here, no device is needed."""
import collections
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "5g-nr-randomaccess_amd")
SHIPPED = os.path.join(PKG, "libprach_hip.so")
NOBITOP3 = os.path.join(PKG, "libprach_hip_nobitop3.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bitop3_inventory.json")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
PHILOX_XOR3 = "0x96"  # a ^ b ^ c: written out on purpose in the Philox rounds (prach_device_fn.h), not a table the compiler chose

SYM = re.compile(r"^[0-9a-f]+ <([^>]+)>:$")
OP = re.compile(r"^\s+(v_bitop3_b(?:16|32))\b([^/]*)")
TABLE = re.compile(r"bitop3:(0x[0-9a-fA-F]+|\d+)")


def demangle(names):
    if not names:  # (c++filt without arguments reads standard input)
        return {}
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    # "void prach::batch_kernel<16, true>(prach::TrialDev const*)" -> "batch_kernel<16, true>"
    return {a: re.sub(r"^void ", "", b.replace("(anonymous namespace)::", "").replace("prach::", "").split("(")[0]) for a, b in zip(names, out)}


def inventory(lib):
    """{kernel: {truth table: sites}} over every gfx950 code object in `lib` (kernels without a site are listed with {})."""
    if not os.path.exists(lib):
        raise FileNotFoundError(f"{lib} is not built (make -C 5g-nr-randomaccess_amd/csrc lib)")
    counts = collections.OrderedDict()
    with tempfile.TemporaryDirectory() as d:
        # llvm-objdump --offloading writes LIB.N.<triple> next to its input: a copy in a directory of our own
        copy = os.path.join(d, os.path.basename(lib))
        shutil.copyfile(lib, copy)
        subprocess.run([OBJDUMP, "--offloading", copy], capture_output=True, text=True, check=True, cwd=d)
        objs = sorted(f for f in os.listdir(d) if f.endswith("gfx950"))
        if not objs:
            raise RuntimeError(f"no gfx950 code object in {lib}")
        for f in objs:
            dis = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.split("\n"):
                m = SYM.match(line)
                if m:
                    cur = m.group(1)
                    counts.setdefault(cur, collections.Counter())
                    continue
                m = OP.match(line)
                if m and cur is not None:
                    t = TABLE.search(m.group(2))
                    counts[cur]["0x%02x" % (int(t.group(1), 0) if t else 0)] += 1
    names = demangle([k for k in counts if k.startswith("_Z")])
    out = {}
    for k, c in counts.items():
        name = names.get(k, k)
        if name in out:  # (one kernel in two code objects: never seen, but not to be lost)
            c = c + collections.Counter(out[name])
        out[name] = dict(sorted(c.items()))
    return dict(sorted(out.items()))


def kernels_with_chosen_tables(inv):
    """The kernels with at least one site of a table other than the Philox xor3: those the GPU cross-check must pin."""
    return sorted(k for k, t in inv.items() if any(tab != PHILOX_XOR3 for tab in t))


def compiler_version():
    p = subprocess.run([HIPCC, "--version"], capture_output=True, text=True)
    return next((l.strip() for l in p.stdout.split("\n") if l.startswith("HIP version")), "unknown")


def diff(old, new):
    """Readable lines for every kernel / table whose count differs (empty: identical)."""
    lines = []
    for k in sorted(set(old) | set(new)):
        a, b = old.get(k), new.get(k)
        if a == b or (a is None and not b):  # (a kernel that is not on file and has no site has no table to put on file: the same as listed with {})
            continue
        if a is None or b is None:
            lines.append(f"{k}: {'new kernel' if a is None else 'kernel gone'} ({a} -> {b})")
            continue
        for t in sorted(set(a) | set(b)):
            if a.get(t, 0) != b.get(t, 0):
                lines.append(f"{k}: table {t}: {a.get(t, 0)} -> {b.get(t, 0)} sites")
    return lines


def table(inv):
    rows = ["| kernel | all | not 0x96 | tables |", "|---|---|---|---|"]
    for k, t in inv.items():
        if t:
            rows.append(f"| `{k}` | {sum(t.values())} | {sum(v for tab, v in t.items() if tab != PHILOX_XOR3)} | "
                        + ", ".join(f"{tab}x{v}" for tab, v in t.items()) + " |")
    return "\n".join(rows)


def main(argv):
    lib = argv[argv.index("--lib") + 1] if "--lib" in argv else SHIPPED
    inv = inventory(lib)
    if "--write" in argv:
        with open(GOLDEN, "w") as f:
            json.dump({"compiler": compiler_version(), "kernels": inv}, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {os.path.relpath(GOLDEN, ROOT)}: {len(inv)} kernels, {len(kernels_with_chosen_tables(inv))} with compiler-chosen tables")
        return 0
    if "--check" in argv:
        with open(GOLDEN) as f:
            old = json.load(f)
        d = diff(old["kernels"], inv)
        print(table(inv))
        if d:
            print(f"\ninventory on file ({old['compiler']}) differs from {os.path.basename(lib)} ({compiler_version()}):\n  " + "\n  ".join(d))
            return 1
        print(f"\nsame as {os.path.relpath(GOLDEN, ROOT)}")
        return 0
    print(table(inv))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
