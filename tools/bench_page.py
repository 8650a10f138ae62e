#!/usr/bin/env python3
"""Measurements behind the page of a row set (cdb_filter, cdb_rowset_page).

Per row count m, count distribution and page end K (decades from 10 to m/2) one JSON line with four timings of "the first K rows
of the ranking", each the host clock around a call that returns with the rows on the host:

  select    cdb_rowset_page(0, K) on a resident row set, the select path forced (debug_page_path = 1)
  sort      the same page, the sort path forced (debug_page_path = 2)
  filter    cdb_filter + cdb_rowset_page(0, K) + cdb_rowset_free: the whole operation, automatic path
  baseline  cdb_query_and_columns(ranked = 1, limit = K) over the same keys — the only way to this page before row sets existed

Every case is warmed up once per path; the repeats are taken turn about between the paths (select, sort, filter, baseline, select,
...), and the median and the range of each are reported.  The keys are a host-rows key that carries the counts and a column that
holds every id, so filter and baseline resolve, upload and merge the same 2 m rows.

Distributions: "equal" (every count 7: no key byte differs), "zipf" (small counts, P(c) ~ 1/c over 1..200: one byte differs),
"three_bytes" (uniform below 2^24: three bytes differ).

--baseline-only measures the baseline alone and needs none of the row-set symbols: run it with --package-root pointing at a built
checkout of the parent commit for the last column of the table in DESIGN.md (its lines say "what": "page_baseline_only").

usage: python tools/bench_page.py [--log2m 16 20 24] [--reps 7] [--baseline-only] [--package-root DIR] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

# --package-root DIR: the tree to import coffeedb_amd (binding and library) from — a checkout of the parent commit for --baseline-only
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in sys.argv:
    _root = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, _root)
from coffeedb_amd import capi  # noqa: E402

LO, HI = 0, 1 << 62


def emit(fp, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if fp:
        fp.write(line + "\n")
        fp.flush()


def counts_of(dist, m, rng):
    if dist == "equal":
        return np.full(m, 7, dtype=np.int64)
    if dist == "zipf":
        w = 1.0 / np.arange(1, 201)
        return (1 + np.searchsorted(np.cumsum(w / w.sum()), rng.random(m), side="right").clip(0, 199)).astype(np.int64)
    return rng.integers(0, 1 << 24, m).astype(np.int64)


def page_ends(m):
    ks, k = [], 10
    while k < m // 2:
        ks.append(k)
        k *= 10
    return ks + [m // 2]


class Keys:
    """the C arrays of [(None, host rows), (column, ["[-inf,inf]"])], made once"""

    def __init__(self, ids, counts, col):
        self.ids, self.counts = ids, counts
        self.arr = (capi.CdbKeyQuery * 1)()
        self.arr[0].ids = ids.ctypes.data
        self.arr[0].counts = counts.ctypes.data
        self.arr[0].nrows = len(ids)
        self.blob, self.offs = capi.GpuColumn._pack(["[-inf,inf]"])
        self.carr = (capi.CdbColumnKey * 1)()
        self.carr[0].column = col._h
        self.carr[0].blob = self.blob.ctypes.data
        self.carr[0].offsets = self.offs.ctypes.data
        self.carr[0].nranges = 1


def baseline(lib, keys, k):
    ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
    rc = lib.cdb_query_and_columns(keys.arr, 1, keys.carr, 1, 1, LO, HI, k, C.byref(ids), C.byref(cnt), C.byref(n))
    if rc != 0:
        raise RuntimeError(f"cdb_query_and_columns failed ({rc})")
    out = (capi._array(ids, n.value, np.int64), capi._array(cnt, n.value, np.int64))
    lib.cdb_free(ids)
    lib.cdb_free(cnt)
    return out


def filter_set(lib, keys):
    h = C.c_void_p()
    rc = lib.cdb_filter(keys.arr, 1, keys.carr, 1, 1, LO, HI, C.byref(h))
    if rc != 0:
        raise RuntimeError(f"cdb_filter failed ({rc})")
    return capi.GpuRowSet(h)


def spread(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2m", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = capi.load_library()
    fp = open(a.out, "a") if a.out else None
    for lg in a.log2m:
        m = 1 << lg
        ids = np.arange(m, dtype=np.int64) * 3 + 1_700_000_000_000  # timestamps
        col = capi.GpuColumn(1, device=0)
        col.add_bulk(ids, np.zeros(m, dtype=np.int64))
        col.build()
        for dist in ("equal", "zipf", "three_bytes"):
            counts = counts_of(dist, m, np.random.default_rng(lg * 10 + len(dist)))
            keys = Keys(ids, counts, col)
            rs = None
            if not a.baseline_only:
                rs = filter_set(lib, keys)
                assert rs.size == m

            def select(k):
                rs.set_option("debug_page_path", 1)
                return rs.page(0, k)

            def sort(k):
                rs.set_option("debug_page_path", 2)
                return rs.page(0, k)

            def whole(k):
                with filter_set(lib, keys) as s:
                    return s.page(0, k)

            paths = [("baseline", lambda k: baseline(lib, keys, k))]
            if not a.baseline_only:
                paths = [("select", select), ("sort", sort), ("filter", whole)] + paths
            for k in page_ends(m):
                want = None
                for name, fn in paths:  # warm-up, and the paths must agree
                    got = fn(k)
                    if want is None:
                        want = got
                    elif not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                        raise RuntimeError(f"{name} disagrees at m = {m}, {dist}, K = {k}")
                ts = {name: [] for name, _ in paths}
                for _ in range(a.reps):
                    for name, fn in paths:
                        t0 = time.perf_counter()
                        fn(k)
                        ts[name].append((time.perf_counter() - t0) * 1e3)
                rec = dict(what="page_baseline_only" if a.baseline_only else "page", m=m, dist=dist, K=k, reps=a.reps, unit="ms")
                for name, _ in paths:
                    rec[name] = spread(ts[name])
                if rs is not None:
                    rec["select_passes"] = int(rs.stat("select_passes"))
                    rec["select_over_sort"] = round(rec["select"]["median"] / rec["sort"]["median"], 4)
                    rec["filter_over_baseline"] = round(rec["filter"]["median"] / rec["baseline"]["median"], 4)
                emit(fp, **rec)
            if rs is not None:
                rs.close()
        col.close()
    if fp:
        fp.close()


if __name__ == "__main__":
    main()
