#!/usr/bin/env python3
"""Is the device code of every kernel the same in two sets of assembly listings?

For a refactor that moves kernels between translation units: the listings are what `make -C coffeedb_amd/csrc isa-scan` writes
(one device `.s` per unit, `hipcc -S --cuda-device-only`).  Every kernel of the BASE listings is looked up in the NEW listings
by its mangled name and two pieces of text are compared, as plain text:
  * the instructions, from the symbol's label to its `.Lfunc_end`, with the numbers of local labels normalised;
  * the `.amdhsa_` resource block (registers, scratch, LDS).
A kernel whose name is not found is looked up once more by its demangled name without `(anonymous namespace)::` — a parameter
type that moved from an anonymous namespace into a header changes the mangled name and nothing else; such kernels are listed.

usage: isa_symbol_compare.py --base parent.s [...] --new unit1.s unit2.s [...]
Exit status 1 when a kernel is missing or differs.
"""
import argparse
import collections
import re
import subprocess
import sys

KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$")
LABEL = re.compile(r"^([^.\s;][^\s:;]*):")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)(\d+)(_\d+)?")


def kernels_of(path):
    """name -> (instruction text, resource block)"""
    with open(path, encoding="utf-8", errors="replace") as f:
        lines = f.read().split("\n")
    label_at = {}
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m:
            label_at.setdefault(m.group(1), i)
    out = {}
    for i, ln in enumerate(lines):
        m = KERNEL.match(ln)
        if not m:
            continue
        name = m.group(1)
        j = i
        while not lines[j].strip().startswith(".end_amdhsa_kernel"):
            j += 1
        res = "\n".join(x.strip() for x in lines[i + 1:j])
        a = label_at[name]
        b = a
        while not lines[b].startswith(".Lfunc_end"):
            b += 1
        out[name] = (lines[a + 1:b], res)
    return out


def normalise(body, name):
    inner = name[2:] if name.startswith("_Z") else name
    text = []
    for ln in body:
        ln = ln.split(";")[0].rstrip()  # (comments carry block numbers and source file names)
        if not ln.strip():
            continue
        ln = ln.replace(name, "<self>").replace(inner, "<self>")
        text.append(LOCAL.sub(lambda m: ".L" + m.group(1) + "#" + (m.group(3) or ""), ln))
    return "\n".join(text)


def demangled(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    base = {}
    for p in a.base:
        base.update(kernels_of(p))
    new = collections.defaultdict(list)  # name -> [(file, body, res)]
    for p in a.new:
        for name, (body, res) in kernels_of(p).items():
            new[name].append((p, body, res))
    by_plain = collections.defaultdict(list)
    for name, plain in demangled(sorted(new)).items():
        by_plain[plain].append(name)
    base_plain = demangled(sorted(base))
    same = renamed = 0
    bad = []
    notes = []
    for name in sorted(base):
        body, res = base[name]
        found = new.get(name)
        other = name
        if not found:
            cands = by_plain.get(base_plain[name], [])
            if len(cands) != 1:
                bad.append(f"MISSING  {name}")
                continue
            other = cands[0]
            found = new[other]
            notes.append(f"RENAMED  {name}\n      -> {other}  [{found[0][0]}]")
            renamed += 1
        if len(found) > 1:
            notes.append(f"TWICE    {name}  in " + ", ".join(f[0] for f in found))
        for path, nbody, nres in found:
            d = []
            if normalise(body, name) != normalise(nbody, other):
                d.append("instructions")
            if res != nres:
                d.append("resource block")
            if d:
                bad.append(f"DIFFERS  {name}  [{path}]: " + " and ".join(d))
        if not any(b.split()[1] == name for b in bad):
            same += 1
    for n in notes + bad:
        print(n)
    print(f"\nkernels in the base listings: {len(base)}; identical in the new listings: {same} (of them found under a changed name: {renamed}); "
          f"missing or different: {len(base) - same}")
    print(f"kernels in the new listings: {sum(len(v) for v in new.values())} ({len(new)} distinct names)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
