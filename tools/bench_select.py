#!/usr/bin/env python3
"""Measurements behind select on the device (cdb_rowset_select, cdb_column_values).  Reports, gates nothing.

Setup: a row set of m = 2^20 rows (cdb_debug_rowset_from_rows, Zipf counts) over two string indexes of m documents of 256 bytes and
four columns (two int64, a double, a bool) of m rows, all holding the same ids.

Per page end K (10, 100, 1000, 10^4 and 10^6, the export case) one JSON line with the host clock around calls that return with the
data on the host, arrays left as the C side returns them (raw = True):

  select        cdb_rowset_select(0, K) with the two string fields (their own keyword lists) and the four columns
  select_str    cdb_rowset_select(0, K) with the two string fields only
  page_render   what the parent offers for the string part: cdb_rowset_page(0, K), then one cdb_render_rows per string field

The column part has no counterpart in the parent (its only way is a host copy of the column), so select_str / page_render is the
comparison and select shows what the four columns add.  One warm-up each, then the repetitions taken turn about; median and range.
A second kind of line ("what": "column_values") times cdb_column_values alone at the same row counts, in rows per second.
--profile adds the kernel times of the last repetition: sel_values next to pg_* (row set) and rnd_* (the first string index).

usage: python tools/bench_select.py [--log2m 20] [--reps 7] [--profile] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi  # noqa: E402

DOC = 256
KW = ([b"abc", b"qz", b"hello"], [b"xy", b"kkk"])
LEFT, RIGHT = b"<b>", b"</b>"


def emit(fp, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if fp:
        fp.write(line + "\n")
        fp.flush()


def spread(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def zipf_counts(m, rng):
    w = 1.0 / np.arange(1, 201)
    return (1 + np.searchsorted(np.cumsum(w / w.sum()), rng.random(m), side="right").clip(0, 199)).astype(np.int64)


def string_index(ids, rng):
    m = len(ids)
    text = rng.integers(ord("a"), ord("z") + 1, m * DOC, dtype=np.uint8)
    ix = capi.GpuStringIndex(0)
    ix.build_view(ids, text, np.arange(m + 1, dtype=np.uint64) * DOC)
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2m", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fp = open(a.out, "a") if a.out else None
    m = 1 << a.log2m
    rng = np.random.default_rng(a.log2m)
    ids = np.arange(m, dtype=np.int64) * 3 + 1_700_000_000_000  # timestamps
    strings = [string_index(ids, rng), string_index(ids, rng)]
    columns = []
    for kind, vals in (("int64", rng.integers(-1 << 40, 1 << 40, m)), ("int64", np.arange(m)), ("double", rng.standard_normal(m)),
                       ("bool", rng.integers(0, 2, m))):
        col = capi.GpuColumn(kind, device=0)
        col.add_bulk(ids, vals)
        col.build()
        columns.append(col)
    rs = capi.debug_rowset_from_rows(ids, zipf_counts(m, rng), device=0)
    if a.profile:
        rs.set_option("profile", 1)
        strings[0].set_option("profile", 1)
    str_fields = [(strings[0], KW[0]), (strings[1], KW[1])]

    def select(k):
        return rs.select(0, k, str_fields + columns, LEFT, RIGHT, raw=True)

    def select_str(k):
        return rs.select(0, k, str_fields, LEFT, RIGHT, raw=True)

    def page_render(k):
        pi, pc = rs.page(0, k)
        return pi, pc, [ix.render_rows(pi, kws, LEFT, RIGHT, spans=False, raw=True) for ix, kws in str_fields]

    paths = [("select", select), ("select_str", select_str), ("page_render", page_render)]
    ends = [k for k in (10, 100, 1000, 10 ** 4, 10 ** 6) if k <= m]
    for k in ends:
        got = {name: fn(k) for name, fn in paths}  # warm-up, and the paths must agree
        for name in ("select", "select_str"):
            assert np.array_equal(got[name][0], got["page_render"][0]) and np.array_equal(got[name][1], got["page_render"][1]), name
            for j in range(2):
                assert got[name][2][j]["text_blob"] == got["page_render"][2][j]["text_blob"], (name, j)
        ts = {name: [] for name, _ in paths}
        for _ in range(a.reps):
            for name, fn in paths:
                t0 = time.perf_counter()
                fn(k)
                ts[name].append((time.perf_counter() - t0) * 1e3)
        rec = dict(what="select", m=m, doc_bytes=DOC, K=k, reps=a.reps, unit="ms", string_fields=2, columns=len(columns))
        for name, _ in paths:
            rec[name] = spread(ts[name])
        rec["select_str_over_page_render"] = round(rec["select_str"]["median"] / rec["page_render"]["median"], 4)
        if a.profile:   # the kernels of ONE more select: the tables add up, so the difference across the call
            before = (rs.profile(), strings[0].profile())
            select(k)
            after = (rs.profile(), strings[0].profile())
            for key, b, c in (("profile_rowset", before[0], after[0]), ("profile_index0", before[1], after[1])):
                rec[key] = {n: round(v["ms"] - b.get(n, {"ms": 0.0})["ms"], 5) for n, v in c.items() if v["launches"] > b.get(n, {"launches": 0})["launches"]}
        emit(fp, **rec)
    for k in ends:
        ask = rng.permutation(ids)[:k].copy()
        columns[0].values(ask)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            columns[0].values(ask)
            ts.append((time.perf_counter() - t0) * 1e3)
        s = spread(ts)
        emit(fp, what="column_values", m=m, rows=k, reps=a.reps, unit="ms", **s, rows_per_s=round(k / (s["median"] * 1e-3)))
    rs.close()
    for x in strings + columns:
        x.close()
    if fp:
        fp.close()


if __name__ == "__main__":
    main()
