#!/usr/bin/env python3
"""Diff two gfx950 assembly files (hipcc -save-temps) kernel by kernel.

  python tools/asm_kernel_diff.py before.s after.s [name-filter] [--rename FROM=TO ...]

Per kernel symbol: instruction counts before and after and whether the instruction streams are
identical; for a kernel that differs, how many lines changed with operands and by mnemonic alone.
Labels, directives and comments are dropped; branch targets keep only their basic-block number, so
that a kernel that merely moved in the file compares equal.  --rename FROM=TO replaces FROM by TO in the symbols of
before.s first: for a kernel whose template parameters changed and whose mangled name therefore did.
"""
import difflib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+|nw_\w+):\s*$", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name], name = body, None
            continue
        s = line.strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def changed(x, y):
    sm = difflib.SequenceMatcher(None, x, y, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def main():
    argv, renames = [], []
    rest = iter(sys.argv[1:])
    for arg in rest:
        if arg == "--rename":
            renames.append(next(rest).split("=", 1))
        else:
            argv.append(arg)
    a, b = kernels(argv[0]), kernels(argv[1])
    for old, new in renames:
        a = {n.replace(old, new): body for n, body in a.items()}
    flt = argv[2] if len(argv) > 2 else ""
    names = sorted(set(a) | set(b))
    pretty = demangle(names)
    differ = 0
    for n in names:
        if flt not in pretty[n]:
            continue
        ia, ib = a.get(n), b.get(n)
        if ia is None or ib is None:
            print(f"{'only before' if ib is None else 'only after':>12}  {pretty[n]}")
            differ += 1
            continue
        if ia == ib:
            print(f"{'identical':>12}  {len(ia):6d} {len(ib):6d}  {pretty[n]}")
            continue
        # with operands (register renaming counts) and by mnemonic alone (the shape of the code)
        full, ops = changed(ia, ib), changed([i.split()[0] for i in ia], [i.split()[0] for i in ib])
        print(f"{'DIFFERS':>12}  {len(ia):6d} {len(ib):6d}  {pretty[n]}  ({full} lines changed, {ops} by mnemonic)")
        differ += 1
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
