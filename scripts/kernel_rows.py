#!/usr/bin/env python3
"""Kernel resource rows of gfx950 code objects, and the rows that differ
between two builds.

  scripts/kernel_rows.py A [A2 ...] --vs B [B2 ...] [--only SUBSTRING]
  scripts/kernel_rows.py A [A2 ...]                  (just the rows)

Each argument is a `hipcc -c` object or a linked library; a side is the union
of the kernels of its files (a kernel split over several units is compared
against the one unit it came from).  Per kernel, from the code object's
metadata note and symbol table only: SGPRs, VGPRs, AGPRs, SGPR and VGPR spill
counts, scratch (private segment) and LDS (group segment) bytes, kernarg bytes,
and the size of the kernel function in bytes.  Nothing is disassembled.

Prints the count of kernels per side, the names on one side only and every row
that differs as `field: (A, B)`; exits 1 when anything differs.  With one side,
prints every row.  Waves per SIMD (512 registers per lane and SIMD, unified
VGPRs + AGPRs in blocks of 8, at most 8) is derived and printed as `waves`."""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ["sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size"]


def code_objects(path):
    """The gfx950 code objects bundled in an object or a library (one per translation unit)."""
    d = open(path, "rb").read()
    if d[:4] == b"\x7fELF" and d[18:20] == struct.pack("<H", 224):  # (EM_AMDGPU: already a code object)
        return [d]
    out, i = [], d.find(MAGIC)
    while i >= 0:
        n, = struct.unpack_from("<Q", d, i + len(MAGIC))
        p = i + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", d, p)
            ident = d[p + 24:p + 24 + idlen]
            p += 24 + idlen
            if ident.startswith(b"hip") and ident.endswith(b"gfx950") and size:
                out.append(d[i + off:i + off + size])
        i = d.find(MAGIC, p)
    if not out:
        sys.exit(f"{path}: no uncompressed gfx950 code object found")
    return out


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def rows_of(path):
    """{mangled kernel name: {field: int}} of every kernel in `path`."""
    rows = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes, syms = tool("llvm-readelf", "--notes", f.name), tool("llvm-readelf", "-sW", f.name)
        size = {}
        for l in syms.split("\n"):
            t = l.split()
            if len(t) == 8 and t[3] == "FUNC":
                size[t[7]] = int(t[2])
        # the metadata is printed as YAML: one "  - " item per kernel under amdhsa.kernels
        body = notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0]
        for item in re.split(r"\n  - ", "\n" + body.strip("\n"))[1:]:
            top = dict(re.findall(r"^(?:    |)\.(\w+): +(\S+)$", item, re.M))
            name = top["name"].strip("'\"")
            rows[name] = {k: int(top[k]) for k in FIELDS if k in top}
            rows[name]["code_bytes"] = size[name]
    return rows


def waves(r):
    regs = -(-r["vgpr_count"] // 8) * 8  # (vgpr_count is the unified total: it includes the AGPRs)
    return min(8, 512 // max(regs, 8))


def side(paths):
    rows = {}
    for p in paths:
        for k, v in rows_of(p).items():
            if k in rows and rows[k] != v:
                sys.exit(f"{p}: {k} is defined twice on one side, with different rows")
            rows[k] = v
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", nargs="+")
    ap.add_argument("--vs", nargs="+", default=[])
    ap.add_argument("--only", default="", help="kernels whose demangled name contains this")
    args = ap.parse_args()
    A, B = side(args.a), side(args.vs)
    names = sorted(set(A) | set(B))
    plain = dict(zip(names, subprocess.run(["c++filt", *names], check=True, capture_output=True,
                                           text=True).stdout.split("\n"))) if names else {}
    names = [n for n in names if args.only in plain[n]]
    if not args.vs:
        for n in names:
            print(plain[n], " ".join(f"{k}={v}" for k, v in A[n].items()), f"waves={waves(A[n])}")
        print(f"{len(names)} kernels")
        return 0
    na, nb = [n for n in names if n in A], [n for n in names if n in B]
    differ = 0
    for n in names:
        if n not in A or n not in B:
            print(f"only in {'A' if n in A else 'B'}: {plain[n]}")
            differ += 1
            continue
        d = {k: (A[n].get(k), B[n].get(k)) for k in list(A[n]) if A[n].get(k) != B[n].get(k)}
        if waves(A[n]) != waves(B[n]):
            d["waves"] = (waves(A[n]), waves(B[n]))
        if d:
            print(plain[n], d)
            differ += 1
    print(f"{len(na)} kernels in A, {len(nb)} in B, {len(set(na) & set(nb))} in both, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
