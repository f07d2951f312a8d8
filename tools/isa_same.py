#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?   isa_same.py BUILD_A BUILD_B

Compares the gfx950 assembly (`make build/<unit>.s` for every unit, in each tree) kernel by kernel: per unit the set of
kernel symbols, and per kernel its instruction text and its .amdhsa_kernel descriptor block (registers, LDS, scratch).
Host-side restructuring reorders template instantiations, which moves kernels inside a file and renumbers the per-function
local labels, so `;` comments are dropped and the function index of local labels (.LBB<n>_, .Lfunc_end<n>) is removed
before the texts are compared.  Prints one row per unit -- unit, kernels, differing -- and exits non-zero on any difference.
"""
import pathlib
import re
import sys

LOCAL = re.compile(r"(\.L[A-Za-z]+?)\d+(_\d+)?\b")  # .LBB12_3 -> .LBB_3, .Lfunc_end12 -> .Lfunc_end


def kernels(path):
    """{symbol: normalised text of the function body and of its descriptor block}"""
    out, sym, part = {}, None, None
    for raw in path.read_text().splitlines():
        line = LOCAL.sub(r"\1\2", raw.split(";", 1)[0]).strip()
        if not line:
            continue
        if m := re.match(r"\.type\s+(\S+),@function", line):
            sym, part = m.group(1), None
            out[sym] = {"body": [], "desc": []}
        elif sym and line == sym + ":":
            part = "body"
        elif m := re.match(r"\.amdhsa_kernel\s+(\S+)", line):
            sym, part = m.group(1), "desc"
        elif line in (".Lfunc_end:", ".end_amdhsa_kernel"):
            part = None
        elif part:
            out[sym][part].append(line)
    return {s: t for s, t in out.items() if t["desc"]}  # kernels only: functions with a descriptor


def main(a, b):
    a, b = pathlib.Path(a), pathlib.Path(b)
    units = sorted({p.name for p in a.glob("*.s")} | {p.name for p in b.glob("*.s")})
    bad = 0 if units else 1
    print(f"{'unit':<34}{'kernels':>8}{'differing':>10}")
    for u in units:
        if not ((a / u).exists() and (b / u).exists()):
            print(f"{u:<34}{'missing in one build':>18}")
            bad += 1
            continue
        ka, kb = kernels(a / u), kernels(b / u)
        diff = sorted(set(ka) ^ set(kb)) + sorted(s for s in set(ka) & set(kb) if ka[s] != kb[s])
        print(f"{u:<34}{len(ka):>8}{len(diff):>10}")
        for s in diff:
            print(f"    {s}")
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
