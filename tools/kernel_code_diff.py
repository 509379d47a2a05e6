#!/usr/bin/env python3
"""Do two builds compile to the same device code?  CPU only, standard library only.

    hipcc <the build's flags> --cuda-device-only -S unit.hip -o unit.s      (once per unit and side)
    tools/kernel_code_diff.py --before old/fa_reduce.s --after new/fa_reduce.s new/fa_rows.s ...

Each assembly file is split at its function labels.  Per mangled symbol the script keeps the
instruction text (comments and assembler directives dropped, local labels renumbered in order of
appearance) and the metadata the assembler and the loader read: the .amdhsa_* lines of the kernel
descriptor, the `.set <symbol>.<key>` resource values, and the scalar keys of the symbol's entry
under amdhsa.kernels (.vgpr_count, .sgpr_count, the spill counts, LDS and scratch sizes, ...).
It prints the symbols found on one side only, the symbols defined in more than one "after" file,
and the symbols whose text or metadata differ, then one summary line; the exit status is non-zero
if any of the three lists is non-empty.

The comparison is equality of text and nothing else: the script knows no instruction by name.
"""
from __future__ import annotations

import argparse
import difflib
import re
import sys
from pathlib import Path

LABEL = re.compile(r"^([A-Za-z_$.][\w$.]*):")
LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?\b")
FUNC_TYPE = re.compile(r"^\.type\s+([\w$.]+),@function")
SET = re.compile(r"^\.set\s+([\w$]+)\.(\w+),\s*(.*)$")


class Function:
    def __init__(self):
        self.text: list[str] = []
        self.meta: dict[str, str] = {}


def renumber(lines):
    """Local labels (.LBB<function>_<block>, .Ltmp<n>, ...) by order of first appearance."""
    names: dict[str, str] = {}
    return [LOCAL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), line) for line in lines]


def parse(path: Path) -> dict[str, Function]:
    funcs: dict[str, Function] = {}
    declared: set[str] = set()
    cur = None  # the function whose body is being read
    lines = path.read_text().split("\n")
    yaml_at = next((i for i, line in enumerate(lines) if line.startswith("amdhsa.kernels:")), len(lines))
    for raw in lines[:yaml_at]:
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if m := FUNC_TYPE.match(line):
            declared.add(m.group(1))
        elif (m := LABEL.match(line)) and m.group(1) in declared and m.group(1) not in funcs:
            cur = funcs[m.group(1)] = Function()
        elif line.startswith(".Lfunc_end"):
            if cur is not None:
                cur.text = renumber(cur.text)
            cur = None
        elif m := SET.match(line):
            if m.group(1) in funcs:
                funcs[m.group(1)].meta[f".set {m.group(2)}"] = renumber([m.group(3)])[0]
        elif cur is not None:
            if line.startswith(".amdhsa_") and not line.startswith(".amdhsa_kernel"):
                key, _, value = line.partition(" ")
                cur.meta[key] = value.strip()
            elif not line.startswith(".") or LABEL.match(line):
                cur.text.append(" ".join(line.split()))
    # amdhsa.kernels: a YAML list of maps; the scalar keys of an entry sit at four spaces
    entry: dict[str, str] = {}

    def close():
        name = entry.pop(".name", None)
        entry.pop(".symbol", None)
        if name in funcs:
            funcs[name].meta.update({f"note {k}": v for k, v in entry.items()})
        entry.clear()

    for raw in lines[yaml_at + 1:]:
        if raw.startswith("  - "):
            close()
            raw = "    " + raw[4:]
        elif not raw.startswith("    "):
            if raw.strip() and not raw.startswith("  "):
                break  # the next top-level key: the kernel list is over
            continue
        if m := re.match(r"^    (\.\w+):\s+(\S.*)$", raw):
            entry[m.group(1)] = m.group(2)
    close()
    return funcs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--before", nargs="+", type=Path, required=True, metavar="FILE.s")
    ap.add_argument("--after", nargs="+", type=Path, required=True, metavar="FILE.s")
    ap.add_argument("--show", type=int, default=20, help="diff lines printed per differing symbol")
    args = ap.parse_args()

    def side(paths):
        merged: dict[str, Function] = {}
        homes: dict[str, list[str]] = {}
        for p in paths:
            for sym, fn in parse(p).items():
                merged.setdefault(sym, fn)
                homes.setdefault(sym, []).append(p.name)
        return merged, homes

    before, _ = side(args.before)
    after, homes = side(args.after)
    only_before = sorted(set(before) - set(after))
    only_after = sorted(set(after) - set(before))
    repeated = sorted(s for s, h in homes.items() if len(h) > 1)
    differ = []
    for sym in sorted(set(before) & set(after)):
        b, a = before[sym], after[sym]
        if b.text != a.text or b.meta != a.meta:
            differ.append(sym)
    for title, syms in (("only before", only_before), ("only after", only_after)):
        for sym in syms:
            print(f"{title}: {sym}")
    for sym in repeated:
        print(f"defined in {len(homes[sym])} after files ({', '.join(homes[sym])}): {sym}")
    for sym in differ:
        b, a = before[sym], after[sym]
        keys = sorted(k for k in set(b.meta) | set(a.meta) if b.meta.get(k) != a.meta.get(k))
        print(f"differs: {sym}")
        for k in keys:
            print(f"    {k}: {b.meta.get(k)} -> {a.meta.get(k)}")
        if b.text != a.text:
            print(f"    instructions: {len(b.text)} -> {len(a.text)}")
            for line in list(difflib.unified_diff(b.text, a.text, "before", "after", lineterm="", n=1))[:args.show]:
                print("      " + line)
    same = len(set(before) & set(after)) - len(differ)
    print(f"kernel_code_diff: {len(before)} device functions before, {len(after)} after in {len(args.after)} "
          f"file(s): {same} equal in text and metadata, {len(differ)} differ, {len(only_before)} only before, "
          f"{len(only_after)} only after, {len(repeated)} defined more than once")
    return 1 if differ or only_before or only_after or repeated else 0


if __name__ == "__main__":
    sys.exit(main())
