#!/usr/bin/env python3
"""Are two device-assembly texts of one translation unit the same code?   python tools/isa_same.py A.s B.s [--map OLD=NEW ...]
(each from `hipcc <the build's flags> --cuda-device-only -S`).  Each text is cut into one piece per kernel symbol -- its section
with the code, the `.amdhsa_*` descriptor and the `.set` resource symbols, and its entry in the metadata (arguments, register
counts, scratch, LDS) -- and the pieces are compared symbol by symbol, whatever order the compiler emitted them in.  Left out of
the comparison: the `__hip_cuid_*` lines (a hash of the source text) and the numbers a function's position in the file gives its
local labels (so two bodies that differ only in WHICH of their own labels a branch names would compare equal: the compiler
numbers labels by position, and a moved block shows in the instructions around it).  --map rewrites a spelling in A's symbols first (a template parameter that left the mangled names).  Exit status 0: same."""
import re
import sys


def pieces(path, maps):
    text = open(path).read()
    for old, new in maps:
        text = text.replace(old, new)
    lines = [l for l in text.split("\n") if "__hip_cuid_" not in l]
    text = re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+", r"\1\2", "\n".join(lines))
    body, meta = text.split("\t.amdgpu_metadata\n")
    out = {}
    body, _, out["tail"] = body.partition("\t.section\t.AMDGPU.gpr_maximums")      # (what follows the last kernel)
    # (a kernel's section line is followed by .globl, or -- template kernels, comdat -- by a .protected line first)
    for chunk in re.split(r"\n(?=\t\.section\t\.text\.\S+\n(?:\t\.protected\t[^\n]*\n)?\t\.globl\t)", "\n" + body)[1:]:
        seen = {}           # labels numbered through the whole file (long-branch targets): by appearance inside the kernel instead
        chunk = re.sub(r"(\.Lpost_getpc)(\d+)", lambda m: m.group(1) + str(seen.setdefault(m.group(2), len(seen))), chunk)
        out["code " + re.search(r"\.globl\t(\S+)", chunk).group(1)] = chunk
    for entry in re.split(r"\n(?=  - \.agpr_count)", meta.split("amdhsa.kernels:\n")[1]):
        out["meta " + re.search(r"\.name:\s+(\S+)", entry).group(1)] = entry
    return out


def main():
    args = sys.argv[1:]
    at = args.index("--map") if "--map" in args else len(args)
    (file_a, file_b), maps = args[:at], [m.split("=", 1) for m in args[at + 1:]]
    a, b = pieces(file_a, maps), pieces(file_b, [])
    differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
    for k in sorted(a.keys() - b.keys()):
        print("only in A:", k)
    for k in sorted(b.keys() - a.keys()):
        print("only in B:", k)
    for k in differ:
        print("differs:", k)
    nk = sum(k.startswith("code ") for k in a)
    print(f"{nk} kernels in A, {sum(k.startswith('code ') for k in b)} in B; "
          f"{len(a.keys() & b.keys()) - len(differ)} of {len(a.keys() | b.keys())} pieces (code + metadata) identical")
    return 1 if differ or a.keys() != b.keys() else 0


if __name__ == "__main__":
    sys.exit(main())
