#!/usr/bin/env python3
"""Measurements behind cdb_column_append and the device path of cdb_column_remove.

Corpus: tools/bench_columns.py's — int64 values, ids = ascending timestamps (the appended rows carry the next timestamps).  Per
row count n and change fraction f one JSON line per operation and contender:

  device   this library, debug_maintain_path = 1 (merge / compaction on the device)
  old      this library, debug_maintain_path = 2 (stage + column_build / host filter + column_build)
  parent   the library of --package-root (a built checkout of the parent commit): cdb_column_add_bulk + cdb_column_build for
           append, its cdb_column_remove for remove; left out without --package-root

Every contender keeps one built column of n rows.  A repeat appends the m = f * n new rows and then removes exactly those rows, so
the column is back at its n rows for the next repeat; both calls are timed with the host clock (they return synchronised).  One
warm-up cycle per contender (rep -1), then --reps cycles taken turn about between the contenders; every cycle leaves a raw
"column_maintain_cycle" line, every (rows, fraction, op, contender) a "column_maintain" line with median (min - max) in ms.  The host
paths at 10^8 rows take seconds per call: --slow-reps (default 3) applies to "old" and "parent" from --slow-from rows on.

usage: python tools/bench_column_maintain.py [--rows 65536 1048576 16777216 100000000] [--fractions 0.0001 0.01 0.5]
           [--kinds int64] [--reps 7] [--package-root DIR] [--out profiles/bench_column_maintain.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coffeedb_amd import capi  # noqa: E402

KINDS = {"bool": 0, "int64": 1, "double": 2}
DTYPES = {0: np.uint8, 1: np.int64, 2: np.float64}


class Column:
    """One cdb_column of one library (this tree's or the parent's), through the plain C ABI."""

    def __init__(self, lib, kind, path, has_append):
        self.lib, self.kind, self.has_append = lib, kind, has_append
        self.h = C.c_void_p()
        assert lib.cdb_column_create(C.byref(self.h), 0, kind) == 0, "no usable device"
        if path is not None:
            self._ok(lib.cdb_debug_column_set_option(self.h, b"debug_maintain_path", path))

    def _ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.cdb_column_last_error(self.h).decode(errors="replace"))

    def build(self, ids, vals):
        self._ok(self.lib.cdb_column_add_bulk(self.h, ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), len(ids)))
        self._ok(self.lib.cdb_column_build(self.h))

    def append(self, ids, vals):
        if self.has_append:
            self._ok(self.lib.cdb_column_append(self.h, ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), len(ids), None))
        else:
            self.build(ids, vals)

    def remove(self, ids):
        removed = C.c_uint64(0)
        self._ok(self.lib.cdb_column_remove(self.h, ids.ctypes.data_as(C.c_void_p), len(ids), C.byref(removed), None))
        assert removed.value == len(ids)

    def rows(self):
        v = C.c_double(0)
        self.lib.cdb_column_get_stat(self.h, b"rows", C.byref(v))
        return int(v.value)

    def close(self):
        self.lib.cdb_column_destroy(self.h)


def declare(lib, has_append):
    vp, u64 = C.c_void_p, C.c_uint64
    lib.cdb_column_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
    lib.cdb_column_destroy.argtypes = [vp]
    lib.cdb_column_destroy.restype = None
    lib.cdb_column_last_error.argtypes = [vp]
    lib.cdb_column_last_error.restype = C.c_char_p
    lib.cdb_column_add_bulk.argtypes = [vp, vp, vp, u64]
    lib.cdb_column_build.argtypes = [vp]
    lib.cdb_column_remove.argtypes = [vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    lib.cdb_column_get_stat.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double)]
    lib.cdb_debug_column_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    if has_append:
        lib.cdb_column_append.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    return lib


def values_of(kind, n, rng):
    if kind == 1:
        return rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    if kind == 2:
        return rng.standard_normal(n)
    return rng.integers(0, 2, n).astype(np.uint8)


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20, 1 << 24, 10 ** 8])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.0001, 0.01, 0.5])
    ap.add_argument("--kinds", nargs="+", default=["int64"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--slow-from", type=int, default=10 ** 8)
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_column_maintain.jsonl"))
    args = ap.parse_args()
    new = declare(capi.load_library(), True)
    libs = [("device", new, 1, True), ("old", new, 2, True)]
    if args.package_root:
        so = os.path.join(os.path.abspath(args.package_root), "coffeedb_amd", "csrc", "libcoffeedb_gpu.so")
        libs.append(("parent", declare(C.CDLL(so), False), None, False))
    rng = np.random.default_rng(1)
    with open(args.out, "a") as fp:
        for kind_name in args.kinds:
            kind = KINDS[kind_name]
            for n in args.rows:
                ids = 1_700_000_000_000 + np.arange(n, dtype=np.int64)   # ascending timestamps
                vals = values_of(kind, n, rng)
                cols = []
                for name, lib, path, has_append in libs:
                    col = Column(lib, kind, path, has_append)
                    col.build(ids, vals)
                    cols.append((name, col))
                for f in args.fractions:
                    m = max(1, int(n * f))
                    nids = ids[-1] + 1 + np.arange(m, dtype=np.int64)
                    nvals = values_of(kind, m, rng)
                    times = {name: {"append": [], "remove": []} for name, _ in cols}
                    reps = {name: (args.slow_reps if n >= args.slow_from and name != "device" else args.reps) for name, _ in cols}
                    for rep in range(-1, args.reps):   # (-1: the warm-up)
                        for name, col in cols:
                            if rep >= reps[name]:
                                continue
                            ta = timed(col.append, nids, nvals)
                            tr = timed(col.remove, nids)
                            assert col.rows() == n
                            fp.write(json.dumps({"what": "column_maintain_cycle", "kind": kind_name, "rows": n, "fraction": f, "changed": m,
                                                 "contender": name, "rep": rep, "append_ms": round(ta, 3), "remove_ms": round(tr, 3)}) + "\n")
                            fp.flush()
                            if rep >= 0:
                                times[name]["append"].append(ta)
                                times[name]["remove"].append(tr)
                    for name, _ in cols:
                        for op in ("append", "remove"):
                            line = json.dumps({"what": "column_maintain", "kind": kind_name, "rows": n, "fraction": f, "changed": m, "op": op,
                                               "contender": name, **summary(times[name][op])})
                            fp.write(line + "\n")
                            fp.flush()
                for _, col in cols:
                    col.close()


if __name__ == "__main__":
    main()
