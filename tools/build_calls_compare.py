"""Did two libraries make the same calls for the same work?

usage: build_calls_compare.py <dir parent> <dir new>
Each directory holds what `rocprofv3 --kernel-trace --hip-trace --stats --output-format csv -d <dir> -o calls -- python
tools/build_calls_script.py` wrote (CDB_LIB_PATH selects the library).  Prints the calls per kernel name and of hipLaunchKernel,
hipMemcpyAsync, hipMemsetAsync and hipStreamSynchronize; exit status 1 when any count differs (every full kernel name, template
arguments included, is compared too)."""
import collections
import csv
import glob
import re
import sys


def counts(d, kind):
    out = collections.Counter()
    files = glob.glob(d + "/**/*" + kind + "_stats.csv", recursive=True)
    assert files, (d, kind)
    for p in files:
        with open(p, newline="") as f:
            for row in csv.DictReader(f):
                out[row["Name"]] += int(row["Calls"])
    return out


def short(name):  # "void cdb::(anonymous namespace)::k<...>(...)" -> "cdb::k"
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.split(r"[<(]", name, 1)[0]


def main():
    a, b = sys.argv[1], sys.argv[2]
    ka, kb = counts(a, "kernel"), counts(b, "kernel")
    full_same = ka == kb
    sa, sb = collections.Counter(), collections.Counter()
    for k, v in ka.items():
        sa[short(k)] += v
    for k, v in kb.items():
        sb[short(k)] += v
    print(f"{'kernel':<50} parent    new")
    for k in sorted(set(sa) | set(sb)):
        print(f"{k:<50} {sa[k]:>6} {sb[k]:>6}" + ("" if sa[k] == sb[k] else "   <-- DIFFERS"))
    ha, hb = counts(a, "hip_api"), counts(b, "hip_api")
    same = full_same
    for k in ("hipLaunchKernel", "hipMemcpyAsync", "hipMemsetAsync", "hipStreamSynchronize"):
        print(f"{k:<50} {ha[k]:>6} {hb[k]:>6}" + ("" if ha[k] == hb[k] else "   <-- DIFFERS"))
        same = same and ha[k] == hb[k]
    print(f"full kernel names (every template instantiation on its own): {len(ka)} parent, {len(kb)} new, "
          + ("equal counts for every one" if full_same else "DIFFERENT: " + str(sorted((set(ka.items()) ^ set(kb.items())))[:10])))
    print("SAME WORK PER CALL" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
