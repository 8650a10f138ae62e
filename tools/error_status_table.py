#!/usr/bin/env python3
"""Every `throw` of the library (coffeedb_amd/csrc, the shim aside), with the status it carries and the status the former
rule gave its text.

The former rule read the message: text starting with "HIP error" was CDB_E_DEVICE, text containing "internal" was
CDB_E_INTERNAL, anything else CDB_E_INVALID.  Now the thrown type carries the status (errors.h).  This script lists, for
every throw statement of the working tree, the string literals of its message, what the former rule makes of them and what
the thrown type says; with --base REV it also checks that REV holds the same messages, file by file and in the same order.

    python3 tools/error_status_table.py --base HEAD~1 > docs/error_status_table.md

Exit status 1 when a row disagrees or a message changed.
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "coffeedb_amd/csrc"
STATUS_OF = {"Error": "Invalid", "DeviceError": "Device", "InternalError": "Internal", "LookbackTimeout": "Internal",
             "RetryWithDenseKeys": "Invalid"}
# Thrown and caught inside the library, never classified: the build's test hook (debug_starve_group = 1) throws only while the
# sort is in XCD-aware tile order, and build_suffix_array catches every LookbackTimeout of such a build and redoes it.
CAUGHT_INSIDE = {"radix sort look-back timed out (test hook)"}
STRING = re.compile(r'"((?:[^"\\]|\\.)*)"')
NAMED = re.compile(r'(?:const\s+char\s*\*\s*|constexpr\s+const\s+char\s*\*\s*|const\s+char\s+)(\w+)(?:\[\])?\s*=\s*((?:"(?:[^"\\]|\\.)*"\s*)+);')


def strip_comments(text):
    """Comments become blanks (line numbers stay); string literals are kept."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == '"':
            j = i + 1
            while j < n and text[j] != '"':
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i))
            i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i)
            j = n if j < 0 else j + 2
            out.append("".join(ch if ch == "\n" else " " for ch in text[i:j]))
            i = j
        else:
            out.append(c)
            i += 1
    return "".join(out)


def former_rule(text):
    if text.startswith("HIP error"):
        return "Device"
    return "Internal" if "internal" in text else "Invalid"


def throws_of(text):
    """(line, thrown type or None for a rethrow, literal text or None when the message is not a literal, note on an explicit status)"""
    code = strip_comments(text)
    bare = STRING.sub(lambda m: '"' + " " * len(m.group(1)) + '"', code)  # (a literal may hold the word throw, or a semicolon)
    named = {m.group(1): "".join(STRING.findall(m.group(2))) for m in NAMED.finditer(code)}
    rows = []
    for m in re.finditer(r"\bthrow\b", bare):
        end = bare.find(";", m.end())
        stmt = code[m.end():end].replace("\\\n", " ")
        line = code.count("\n", 0, m.start()) + 1
        stmt = " ".join(stmt.split())
        if not stmt:
            rows.append((line, None, None, None))
            continue
        t = re.match(r"(?:::)?(?:cdb::)?((?:std::)?\w+)\s*\((.*)\)$", stmt)
        if not t:
            raise SystemExit(f"cannot read the throw at line {line}: {stmt}")
        typ, args = t.group(1), t.group(2)
        lits = STRING.findall(args)
        if not lits:
            ident = re.search(r"\b(\w+)\b(?!\s*\()", re.sub(r"\b(?:std::string|Status::\w+|Status)\b", "", args))
            if ident and ident.group(1) in named:
                lits = [named[ident.group(1)]]
        given = "the code passed in" if args.startswith("(Status)") else None
        rows.append((line, typ, " … ".join(lits) if lits else None, given))
    return rows


def sources():
    for name in sorted(os.listdir(os.path.join(ROOT, CSRC))):
        if name.endswith((".hip", ".h")):
            yield f"{CSRC}/{name}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", help="a revision whose messages must equal the working tree's")
    a = ap.parse_args()
    bad = 0
    print("| file:line | thrown | message literals | former rule | status carried |")
    print("|---|---|---|---|---|")
    for path in sources():
        with open(os.path.join(ROOT, path), encoding="utf-8") as f:
            rows = throws_of(f.read())
        for line, typ, lit, given in rows:
            if typ is None:
                continue  # `throw;` passes the exception on unchanged
            if typ.startswith("std::"):
                carried = {"std::bad_alloc": "Device (\"out of host memory\")"}.get(typ, "not an Error: Internal")
                print(f"| {path}:{line} | {typ} | {lit or ''} | — | {carried} |")
                continue
            if typ not in STATUS_OF:
                raise SystemExit(f"{path}:{line}: unknown error type {typ}")
            if lit is None:
                print(f"| {path}:{line} | {typ} | (no literal: passes a message on) | — | {STATUS_OF[typ] if given is None else given} |")
                continue
            old, new = former_rule(lit), STATUS_OF[typ]
            note = ""
            if lit in CAUGHT_INSIDE:
                note = " (caught inside the library, never reaches the boundary)"
            elif old != new:
                bad += 1
                note = " **differs**"
            print(f"| {path}:{line} | {typ} | `{lit}` | {old} | {new}{note} |")
        if a.base:
            try:
                base = subprocess.check_output(["git", "-C", ROOT, "show", f"{a.base}:{path}"], text=True, stderr=subprocess.DEVNULL)
            except subprocess.CalledProcessError:
                continue  # a new file
            was = [r[2] for r in throws_of(base) if r[1] and r[2] is not None]
            now = [r[2] for r in rows if r[1] and r[2] is not None]
            if was != now:
                bad += 1
                print(f"\n**{path}: the messages differ from {a.base}**\n", file=sys.stdout)
                for x in was:
                    if x not in now:
                        print(f"- gone: `{x}`")
                for x in now:
                    if x not in was:
                        print(f"- new: `{x}`")
    print(f"\n{'All rows agree.' if not bad else str(bad) + ' disagreements.'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
