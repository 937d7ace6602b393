#!/usr/bin/env python3
"""Count the instructions of one kernel in the gfx950 assembly of a .hip file, by class.

    tools/isa_count.py bwa-mem-scale_amd/csrc/bsw_extend.hip bsw_pk_kernel \
        --begin BSW_PK_PASS_BEGIN --end BSW_PK_PASS_END [-D NAME ...] [--keep out.s]

The file is compiled device-only to assembly with the flags of csrc/Makefile.  For the kernel whose (mangled) symbol
contains the given name the tool prints the number of instructions by mnemonic prefix (v_pk_, other v_, s_nop, other s_,
ds_, global_, the rest) for the whole function and, when two marker comments are named, for the lines between them in
the order of the text (a block the compiler has laid out elsewhere is counted where it lies).  A marker is an assembly
comment put into the source with `asm volatile("; NAME")`.  --list prints the counted lines of the marked region.

The classes are mnemonic prefixes and nothing else: the tool makes no statement about any particular instruction."""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("v_pk_", "v_", "s_nop", "s_", "ds_", "global_", "other")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def compile_asm(src: str, defines: list[str], arch: str, hipcc: str, out: str) -> None:
    cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={arch}", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include")]
    cmd += ["-D" + d for d in defines] + [src, "-o", out]
    subprocess.check_call(cmd)


def classify(mnemonic: str) -> str:
    for c in CLASSES[:-1]:
        if mnemonic.startswith(c):
            return c
    return "other"


def kernel_lines(text: list[str], name: str) -> list[str]:
    """The lines of the function whose label contains `name`, from its label to its .Lfunc_end."""
    start = None
    for n, line in enumerate(text):
        if start is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and name in m.group(1) and not m.group(1).startswith(".L"):
                start = n + 1
        elif line.startswith(".Lfunc_end"):
            return text[start:n]
    raise SystemExit(f"no function whose symbol contains {name!r}" if start is None else f"{name}: no .Lfunc_end")


def count(lines: list[str]) -> tuple[Counter, list[str]]:
    c: Counter = Counter()
    kept = []
    for line in lines:
        body = line.split(";", 1)[0]
        if not body.strip() or body.lstrip().startswith(".") or body.rstrip().endswith(":"):
            continue
        m = INSN.match(body)
        if m:
            c[classify(m.group(1))] += 1
            kept.append(line.rstrip())
    return c, kept


def between(lines: list[str], begin: str, end: str) -> list[str]:
    def find(tag: str) -> int:
        hits = [n for n, line in enumerate(lines) if re.match(rf"^\s*;\s*{re.escape(tag)}\s*$", line)]
        if len(hits) != 1:
            raise SystemExit(f"marker {tag!r}: {len(hits)} occurrences in the kernel, one expected")
        return hits[0]
    b, e = find(begin), find(end)
    if b < e:
        return lines[b + 1:e]
    # The markers enclose the body of a loop that the compiler has rotated: the blocks that end the body lie in front of the
    # loop's header.  The region is then the text from the first marker to the end of the loop's blocks, and from the loop's
    # first block to the second marker.  The loop is the one the label comments name ("in Loop: Header=BBn_m").
    labels = [(n, re.match(r"^(\.LBB\d+_\d+):\s*(?:;\s*(.*))?$", line)) for n, line in enumerate(lines)]
    labels = [(n, m.group(1), m.group(2) or "") for n, m in labels if m]
    own = [x for x in labels if x[0] < b]
    if not own:
        raise SystemExit(f"marker {end!r} lies before {begin!r} in the text, and {begin!r} is in no labelled block")
    m = re.search(r"Header=(BB\d+_\d+) Depth=1\b", own[-1][2])
    head = m.group(1) if m else own[-1][1][2:]
    inside = [k for k, x in enumerate(labels) if x[1] == ".L" + head or re.search(rf"\b{head} Depth=1\b", x[2])]
    if not inside:
        raise SystemExit(f"marker {end!r} lies before {begin!r} in the text, and no loop around them was found")
    first = labels[inside[0]][0]
    last = labels[inside[-1] + 1][0] if inside[-1] + 1 < len(labels) else len(lines)
    if not first <= e < b < last:
        raise SystemExit("the markers do not lie in one loop")
    print(f"(loop {head} is rotated: counting from {begin} to the end of its blocks and from its first block to {end})")
    return lines[b + 1:last] + lines[first:e]


def show(title: str, c: Counter) -> None:
    vec = c["v_pk_"] + c["v_"]
    print(f"{title}: {sum(c.values())} instructions, {vec} vector (v_pk_ + v_)")
    print("  " + "  ".join(f"{k} {c[k]}" for k in CLASSES))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source", help="a .hip file, or with --asm an assembly file already made")
    ap.add_argument("kernel", help="a substring of the kernel's symbol")
    ap.add_argument("--begin"), ap.add_argument("--end")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--asm", action="store_true", help="the source is assembly: do not compile")
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("--list", action="store_true", help="print the counted lines of the marked region")
    a = ap.parse_args()
    if bool(a.begin) != bool(a.end):
        ap.error("--begin and --end go together")
    if a.asm:
        path = a.source
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="isa_count_"), "out.s")
        compile_asm(a.source, a.defines, a.arch, a.hipcc, path)
    with open(path) as f:
        text = f.read().split("\n")
    fn = kernel_lines(text, a.kernel)
    show(f"{a.kernel}, whole function", count(fn)[0])
    if a.begin:
        c, kept = count(between(fn, a.begin, a.end))
        show(f"{a.kernel}, {a.begin} .. {a.end}", c)
        if a.list:
            print("\n".join(kept))
    return 0


if __name__ == "__main__":
    sys.exit(main())
