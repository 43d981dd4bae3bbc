#!/usr/bin/env python3
"""
Compare two device assembly listings function by function.

    python scripts/dev/compare_device_asm.py A.s B.s

A.s and B.s are `hipcc --cuda-device-only -S` outputs of csrc/codd_knn.hip (the flags of build.HIPCC_FLAGS without -shared).
Each listing is split into functions by mangled name: a function is everything from its `.type NAME,@function` line to its
`; -- End function` line, plus the resource lines the compiler prints behind it (`.set NAME.num_vgpr, ...`, `; Kernel info:`).
Local labels carry the function's position in the file: block labels (.LBB12_3, and BB12_3 in the loop comments) lose that
number, the others (.Lfunc_end12, .Ltmp40) are renumbered by first appearance inside the function, and the padding in front
of a comment, which depends on the label's length, is collapsed, so that moving a definition does not count as a difference.

Not compared: what stands outside the functions — the .amdhsa_kernel descriptors are inside and are compared, but the
.amdgpu_metadata block at the end of the listing (kernarg layout, LDS and private sizes per kernel, in file order), LDS and
other data symbols, and the order of the functions (reported, not counted as a difference) are not.

Prints how many functions each file has, which exist in one only and which differ (demangled); exits 1 on any difference.
Reads the two files and nothing else.
"""

from __future__ import annotations

import re
import subprocess
import sys

_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function\s*$")
_END = re.compile(r"^\s*;\s*-- End function\s*$")
_TRAILER = re.compile(r"^\s*(\.set\s|;|\.section\s+\.AMDGPU\.csdata|\.text\s*$|$)")
_LABEL = re.compile(r"\.L[A-Za-z0-9_$]+")
_BLOCK = re.compile(r"(\.L|\b)BB\d+_(\d+)")
_COMMENT_PAD = re.compile(r"\s+;")


def functions(text: str) -> dict[str, list[str]]:
    """mangled name -> its lines, local labels renumbered, trailing blanks dropped"""
    out: dict[str, list[str]] = {}
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = _TYPE.match(lines[i])
        if not m:
            i += 1
            continue
        name, body = m.group(1), []
        while i < len(lines):
            body.append(lines[i])
            i += 1
            if _END.match(body[-1]):
                break
        while i < len(lines) and _TRAILER.match(lines[i]) and not _TYPE.match(lines[i]):
            body.append(lines[i])
            i += 1
        labels: dict[str, str] = {}

        def renumber(t):
            return t.group(0) if t.group(0).startswith(".LBB_") else labels.setdefault(t.group(0), ".L%d" % len(labels))

        # block labels, in code (.LBB12_3) and in the loop comments (Header=BB12_3), lose the function's number; the other local
        # labels are renumbered; the padding in front of a comment depends on the label's length
        body = [_LABEL.sub(renumber, _COMMENT_PAD.sub(" ;", _BLOCK.sub(r"\1BB_\2", line.rstrip()))) for line in body]
        while body and (not body[-1] or body[-1].lstrip().startswith((".section", ".text"))):
            body.pop()
        if name in out:
            raise SystemExit(f"{name} is defined twice in one listing")
        out[name] = body
    return out


def demangle(names: list[str]) -> dict[str, str]:
    if not names:
        return {}
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            res = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True)
        except OSError:
            continue
        got = res.stdout.splitlines()
        if res.returncode == 0 and len(got) == len(names):
            return dict(zip(names, got))
    return {n: n for n in names}


def main(argv: list[str]) -> int:
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    a, b = (functions(open(p, encoding="utf-8", errors="replace").read()) for p in argv[1:])
    only_a = [n for n in a if n not in b]
    only_b = [n for n in b if n not in a]
    differ = [n for n in a if n in b and a[n] != b[n]]
    pretty = demangle(only_a + only_b + differ)
    print(f"{argv[1]}: {len(a)} functions")
    print(f"{argv[2]}: {len(b)} functions")
    for title, names in ((f"only in {argv[1]}", only_a), (f"only in {argv[2]}", only_b), ("differ", differ)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("   ", pretty[n])
    print("same order" if list(a) == list(b) else "order of functions differs")
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
