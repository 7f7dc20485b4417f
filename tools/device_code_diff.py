#!/usr/bin/env python3
"""Compare the gfx950 device code of two build trees: python tools/device_code_diff.py LIB_A LIB_B (two lib/ directories of objects).

For every *.o that carries a .hip_fatbin section the code object is unbundled and compared: the bytes of .text and of .rodata (the kernel
descriptors), and per kernel the metadata note -- register counts, spills, LDS and private segment sizes, the kernarg layout.  Prints what
differs; the exit status is 1 on any difference (an object missing on one side included), else 0.  What a refactor of host code or of shared
headers must leave alone is exactly this.  Where the sections differ but every kernel's own bytes do not -- its code, and its descriptor apart from
the distance between the two -- the kernels only stand in another order (the order their instances are first named in the source), and the report says so."""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def device_code(obj, tmp):
    """None for an object without device code, else ({section: bytes}, {kernel: its metadata text})."""
    if ".hip_fatbin" not in _run("llvm-readelf", "-S", obj):
        return None
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    _run("llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "unused.o"))
    _run("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    sections = {}
    for sec in (".text", ".rodata"):
        out = os.path.join(tmp, "sec.bin")
        if os.path.exists(out):
            os.remove(out)
        _run("llvm-objcopy", "--dump-section", f"{sec}={out}", co, os.path.join(tmp, "unused.co"))
        sections[sec] = open(out, "rb").read()
    notes = _run("llvm-readelf", "--notes", co)
    body = notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0] if "amdhsa.kernels:" in notes else ""
    kernels = {}
    for entry in re.split(r"^  - ", body, flags=re.M)[1:]:
        kernels[re.search(r"\.name:\s*(\S+)", entry).group(1)] = entry
    return sections, kernels, _own_bytes(co, sections)


def _own_bytes(co, sections):
    """{symbol: bytes} of every kernel (.text) and kernel descriptor (.rodata; without bytes 16-23, the offset from the descriptor to the code)"""
    base = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"\] (\.text|\.rodata)\s+PROGBITS\s+([0-9a-f]+)", _run("llvm-readelf", "-S", "-W", co))}
    own = {}
    for m in re.finditer(r"^\s*\d+: ([0-9a-f]+)\s+(\d+) (FUNC|OBJECT)\s+\S+\s+\S+\s+\d+ (\S+)$", _run("llvm-readelf", "--dyn-syms", "-W", co), flags=re.M):
        if m.group(3) == "OBJECT" and not m.group(4).endswith(".kd"):
            continue
        sec = ".text" if m.group(3) == "FUNC" else ".rodata"
        at = int(m.group(1), 16) - base[sec]
        b = sections[sec][at:at + int(m.group(2))]
        own[m.group(4)] = b if sec == ".text" else b[:16] + b[24:]
    return own


def _fields(entry):
    """scalar members of a kernel's metadata; the argument list as one member"""
    head, _, rest = entry.partition(".args:")
    args, _, tail = rest.partition("    .group_segment_fixed_size")
    d = dict(re.findall(r"^\s*(\.\w+):\s*(\S+)\s*$", head + "\n    .group_segment_fixed_size" + tail, flags=re.M))
    d[".args"] = " ".join(args.split())
    return d


def main(a, b):
    names = sorted({os.path.basename(p) for d in (a, b) for p in glob.glob(os.path.join(d, "*.o"))})
    bad = compared = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            pa, pb = os.path.join(a, name), os.path.join(b, name)
            ca = device_code(pa, tmp) if os.path.exists(pa) else None
            cb = device_code(pb, tmp) if os.path.exists(pb) else None
            if ca is None and cb is None:
                continue                                              # a host object (on the side that has it)
            if ca is None or cb is None:
                print(f"{name}: device code on one side only")
                bad += 1
                continue
            compared += 1
            diffs = [f"{sec} differs ({len(ca[0][sec])} / {len(cb[0][sec])} bytes)" for sec in ca[0] if ca[0][sec] != cb[0][sec]]
            for k in sorted(set(ca[1]) | set(cb[1])):
                if k not in ca[1] or k not in cb[1]:
                    diffs.append(f"kernel {k}: on one side only")
                elif ca[1][k] != cb[1][k]:
                    fa, fb = _fields(ca[1][k]), _fields(cb[1][k])
                    what = ", ".join(f"{f} {fa.get(f)} -> {fb.get(f)}" for f in sorted(set(fa) | set(fb)) if fa.get(f) != fb.get(f))
                    diffs.append(f"kernel {k}: {what or 'metadata text differs'}")
            if diffs and all(d.startswith(".") for d in diffs) and ca[2] == cb[2]:
                diffs.append(f"each of the {len(ca[1])} kernels and its descriptor is byte-identical: the kernels stand in another order")
            if diffs:
                bad += 1
                print(f"{name}: DIFFERENT\n  " + "\n  ".join(diffs))
            else:
                print(f"{name}: identical ({len(ca[1])} kernels, {len(ca[0]['.text'])} bytes of .text)")
    print(f"{compared} kernel objects compared, {bad} differ")
    return 1 if bad or not compared else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
