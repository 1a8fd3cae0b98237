#!/usr/bin/env python3
"""Compare two gfx950 code objects kernel by kernel:  code_object_diff.py A.hsaco B.hsaco

The build is deterministic, so a refactor that is meant to leave the device code alone can be held to the strictest test
there is: the code object it builds is the one its parent builds, byte for byte.  This tool says so -- or says which
kernels moved.  It reports

  * whether the two files are identical (then nothing else is looked at);
  * per kernel symbol, whether its code bytes differ (value and size from `llvm-readelf --symbols`, the bytes cut out of
    the .text section that `llvm-objcopy --dump-section` writes);
  * per kernel, which of the resource figures of the metadata note (`llvm-readelf --notes`) differ: registers, LDS,
    private memory, kernel arguments, spills;
  * kernels that only one of the files has.

It compares bytes and numbers; it does not disassemble.  Exit status 0 only when nothing differs.
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
META_FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
               ".kernarg_segment_size", ".vgpr_spill_count", ".sgpr_spill_count")


def _tool(name: str) -> str:
    path = os.path.join(LLVM_BIN, name)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found (set LLVM_BIN)")
    return path


def sha256(path: str) -> str:
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def text_section(path: str):
    """(address, file offset, size) of .text from the section headers."""
    out = subprocess.check_output([_tool("llvm-readelf"), "--section-headers", "--wide", path], text=True)
    for line in out.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[1] == ".text":
            return int(f[3], 16), int(f[4], 16), int(f[5], 16)
    raise RuntimeError(f"{path}: no .text section")


def kernel_symbols(path: str) -> dict:
    """name -> (value, size) of every kernel: a FUNC symbol with its kernel descriptor `<name>.kd` next to it (a device function
    that survived inlining has none)."""
    out = subprocess.check_output([_tool("llvm-readelf"), "--symbols", "--wide", path], text=True)
    funcs, names = {}, set()
    for line in out.splitlines():
        f = line.split()
        if len(f) == 8:
            names.add(f[7])
            if f[3] == "FUNC":
                funcs[f[7]] = (int(f[1], 16), int(f[2]))
    return {n: v for n, v in funcs.items() if n + ".kd" in names}


def text_bytes(path: str) -> bytes:
    with tempfile.TemporaryDirectory() as d:
        dump = os.path.join(d, "text.bin")
        subprocess.check_call([_tool("llvm-objcopy"), f"--dump-section=.text={dump}", path, os.path.join(d, "copy.hsaco")])
        with open(dump, "rb") as f:
            return f.read()


def kernel_metadata(path: str) -> dict:
    """kernel name -> {field: number} for META_FIELDS, from the amdhsa metadata note.

    The note is YAML: `amdhsa.kernels:` is a list whose entries open with `- ` at one indent and keep their own keys two columns
    further in; deeper lines (the entries of `.args`, the two numbers of `.language_version`) belong to those keys and are passed over."""
    out = subprocess.check_output([_tool("llvm-readelf"), "--notes", path], text=True)
    meta, cur = {}, None
    dash = None  # the indent of the kernel list's `- `, known from its first entry
    inside = False
    for line in out.splitlines():
        body = line.lstrip(" ")
        indent = len(line) - len(body)
        if not inside:
            inside = body.startswith("amdhsa.kernels:")
            continue
        if not body:
            continue
        if dash is None:
            if not body.startswith("- "):
                break  # an empty list
            dash = indent
        if indent < dash or (indent == dash and not body.startswith("- ")):
            break  # the next top-level key of the note: the list is over
        if indent == dash:  # a new kernel; its first key stands on the same line
            cur = {}
            body, indent = body[2:], indent + 2
        if indent != dash + 2:
            continue
        key, sep, val = body.partition(":")
        key, val = key.strip(), val.strip()
        if not sep:
            continue
        if key in META_FIELDS:
            cur[key] = int(val)
        elif key == ".name":
            meta[val] = cur
    return meta


def compare(a: str, b: str, out=sys.stdout) -> int:
    ha, hb = sha256(a), sha256(b)
    print(f"A {ha}  {a}", file=out)
    print(f"B {hb}  {b}", file=out)
    if ha == hb:
        print("identical", file=out)
        return 0
    print("the files differ", file=out)
    sa, sb = kernel_symbols(a), kernel_symbols(b)
    ta, tb = text_bytes(a), text_bytes(b)
    (aa, _, _), (ab, _, _) = text_section(a), text_section(b)
    ma, mb = kernel_metadata(a), kernel_metadata(b)
    differing = 0
    for name in sorted(set(sa) | set(sb)):
        if name not in sa or name not in sb:
            print(f"only in {'A' if name in sa else 'B'}: {name}", file=out)
            differing += 1
            continue
        (va, na), (vb, nb) = sa[name], sb[name]
        what = []
        if ta[va - aa:va - aa + na] != tb[vb - ab:vb - ab + nb]:
            what.append(f"code differs ({na} / {nb} bytes)")
        fa, fb = ma.get(name, {}), mb.get(name, {})
        for side, fields in (("A", fa), ("B", fb)):
            absent = [f for f in META_FIELDS if f not in fields]
            if absent:  # never compare a figure that was not read
                what.append(f"metadata of {side} lacks {', '.join(absent)}")
        for f in META_FIELDS:
            if fa.get(f) != fb.get(f):
                what.append(f"{f} {fa.get(f)} / {fb.get(f)}")
        if what:
            print(f"{name}: " + "; ".join(what), file=out)
            differing += 1
    print(f"{differing} of {len(set(sa) | set(sb))} kernels differ" if differing else
          "no kernel differs in code or resources: the difference lies outside .text and the resource figures", file=out)
    return 1


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    return compare(argv[1], argv[2])


if __name__ == "__main__":
    sys.exit(main(sys.argv))
