#!/usr/bin/env python3
"""Do two builds of rayhip.hip hold the same device code?  For a change that is meant to touch host code only.

    python tools/compare_code_objects.py <parent>/rayhip.o <branch>/rayhip.o

Unbundles the gfx950 code object from each object file (section .hip_fatbin, clang-offload-bundler) and compares
  * .text, .rodata (the kernel descriptors) and .note (per-kernel VGPRs, SGPRs, LDS, scratch) byte for byte;
  * where functions only moved -- kernels are emitted in the order the host code first names them -- every symbol's size and bytes instead
    (of a kernel descriptor all but bytes 16..23, the offset to its kernel's code, which is checked to point at that kernel), and the per-kernel
    entries of the metadata note (arguments, registers, LDS, scratch, spills);
  * the symbol lists;
  * for every kernel whose bytes differ, its size in both builds and the difference of its mnemonic counts (llvm-objdump -d
    --disassemble-symbols=<kernel>, the first field of each instruction line), or "none": a kernel that only took other registers or
    another operand order holds the same multiset of instructions.
Exit status 0 when no kernel differs.  Needs no GPU."""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

import yaml


def llvm(tool):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    return shutil.which(tool) or tool


def sh(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def unbundle(obj, out_dir):
    fat, co = os.path.join(out_dir, "fatbin"), os.path.join(out_dir, "gfx950.co")
    sh(llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    sh(llvm("clang-offload-bundler"), "--type=o", "--unbundle", f"--input={fat}", f"--output={co}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950")
    return co


def section_table(co):
    tab = {}
    for line in sh(llvm("llvm-readelf"), "-S", "-W", co).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            tab[m.group(1)] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16))
    return tab


def symbols(co):
    syms = {}
    for line in sh(llvm("llvm-readelf"), "-s", "-W", co).splitlines():
        m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+(\S+)\s+(\S+)$", line)
        if m:
            syms[m.group(5)] = (int(m.group(1), 16), int(m.group(2)), m.group(3), m.group(4))
    return syms


def kernel_notes(co):
    out = sh(llvm("llvm-readelf"), "--notes", co)
    meta = yaml.safe_load(out[out.index("---"):out.rindex("...")])
    return {k[".symbol"]: k for k in meta["amdhsa.kernels"]}


class CodeObject:
    def __init__(self, obj, tmp):
        self.path = unbundle(obj, tmp)
        self.raw = open(self.path, "rb").read()
        self.sections, self.symbols, self.notes = section_table(self.path), symbols(self.path), kernel_notes(self.path)

    def section(self, name):
        for sec, _, off, size in self.sections.values():
            if sec == name:
                return self.raw[off:off + size]
        return b""

    def body(self, sym):
        addr, size, _, ndx = self.symbols[sym]
        if ndx not in self.sections or size == 0 or self.sections[ndx][0] == ".bss":
            return None
        _, saddr, off, _ = self.sections[ndx]
        return self.raw[off + addr - saddr:off + addr - saddr + size]


def mnemonic_counts(co, kernel):
    """the multiset of instruction mnemonics of one kernel: the first field of every instruction line of its disassembly"""
    counts = collections.Counter()
    for line in sh(llvm("llvm-objdump"), "-d", f"--disassemble-symbols={kernel}", co).splitlines():
        if line.startswith(("\t", " ")) and line.split():
            counts[line.split()[0]] += 1
    return counts


def note_differences(x, y):
    """the scalar fields of two per-kernel note entries that differ, as 'field a -> b'"""
    x, y = x or {}, y or {}
    out = []
    for f in sorted(set(x) | set(y)):
        if x.get(f) != y.get(f):
            is_list = isinstance(x.get(f, y.get(f)), list)  # (.args and the like: named, not printed)
            out.append(f"{f} (list field)" if is_list else f"{f} {x.get(f)} -> {y.get(f)}")
    return out


def main(obj_a, obj_b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        return compare(CodeObject(obj_a, ta), CodeObject(obj_b, tb))


def compare(a, b):
    for sec in (".text", ".rodata", ".note"):
        x, y = a.section(sec), b.section(sec)
        print(f"{sec}: {'identical' if x == y else 'differs'} ({len(x)} / {len(y)} bytes, sha256 {hashlib.sha256(x).hexdigest()[:16]} / {hashlib.sha256(y).hexdigest()[:16]})")
    cuid = re.compile(r"__hip_cuid_[0-9a-f]+")
    only_a = sorted(s for s in set(a.symbols) - set(b.symbols) if not cuid.fullmatch(s))
    only_b = sorted(s for s in set(b.symbols) - set(a.symbols) if not cuid.fullmatch(s))
    print(f"symbols: {len(a.symbols)} / {len(b.symbols)}; only in the first: {only_a}; only in the second: {only_b}")
    common = sorted(set(a.symbols) & set(b.symbols))
    moved = sum(1 for s in common if a.symbols[s][0] != b.symbols[s][0])
    differ = []
    for s in common:
        if a.symbols[s][1] != b.symbols[s][1]:
            differ.append(s + " (size)")
            continue
        x, y = a.body(s), b.body(s)
        if s.endswith(".kd") and x and y and s[:-3] in a.symbols:
            for co, d in ((a, x), (b, y)):  # the descriptor points at its kernel
                if co.symbols[s][0] + int.from_bytes(d[16:24], "little", signed=True) != co.symbols[s[:-3]][0]:
                    differ.append(s + " (entry offset)")
            x, y = x[:16] + x[24:], y[:16] + y[24:]
        if x != y:
            differ.append(s)
    kernels = sum(1 for s in common if a.symbols[s][2] == "FUNC")
    print(f"common symbols: {len(common)}, {kernels} of them functions; at another address: {moved}; size or bytes differ: {differ}")
    # every kernel whose bytes differ: its size in both builds, and what the two builds' multisets of mnemonics do not share
    for s in sorted({d.split(" ")[0] for d in differ}):
        if a.symbols[s][2] != "FUNC":
            continue
        ca, cb = mnemonic_counts(a.path, s), mnemonic_counts(b.path, s)
        delta = ", ".join(f"{m} {cb[m] - ca[m]:+d}" for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m])
        print(f"  {s}: {a.symbols[s][1]} / {b.symbols[s][1]} bytes; mnemonic counts: {delta or 'none'}")
    notes_equal = a.notes == b.notes
    print(f"kernels in the metadata note: {len(a.notes)} / {len(b.notes)}; per-kernel entries equal: {notes_equal}")
    for k in sorted(set(a.notes) | set(b.notes)):
        if a.notes.get(k) != b.notes.get(k):
            print("  differs:", k, "--", "; ".join(note_differences(a.notes.get(k), b.notes.get(k))))
    return 0 if not differ and not only_a and not only_b and notes_equal else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
