#!/usr/bin/env python3
"""Measurements behind cdb_rowset_remove and cdb_rowset_all.

Database: two string indexes of --docs documents of --doclen bytes (printable ASCII) plus an int64 and a double column over the
same ids.  For a set of a share of the ids, held as a row set on the device (the state a cdb_filter leaves), it records, as the
caller sees them through the Python binding:
  (a) removal   new: one cdb_rowset_remove over the four fields.  old: cdb_rowset_rows (every id comes down) and then one
                cdb_remove / cdb_column_remove per field (each uploads the ids again) through the SAME library: that path is
                unchanged, so it is the comparison, not the code under test.  The two are alternated --reps times; the four fields are
                rebuilt before every timed call (not timed).  Median (min - max).
  (b) memory    the allocator's peak above the in-use level in front of the call, for both ways (the new call holds every field's
                new column beside its old one at the same time).
  (c) union     cdb_rowset_all over the four fields, over one field alone (the path without a sort), and the host way: np.unique
                over the concatenated id lists the caller would hold, then the row set uploaded (cdb_debug_rowset_from_rows).

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_rowset_remove.py [--docs 1048576] [--doclen 256] [--reps 7] [--shares 0.001,0.1] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi, workloads as W  # noqa: E402


def emit(fp, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if fp:
        fp.write(line + "\n")
        fp.flush()


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def mib(ts):
    return {"median_mib": round(float(np.median(ts)) / 2**20, 1), "min_mib": round(min(ts) / 2**20, 1), "max_mib": round(max(ts) / 2**20, 1)}


class Fields:
    def __init__(self, docs, doclen):
        self.ids = np.arange(docs, dtype=np.int64) * 7 + 1000
        self.blobs = [W.ascii_corpus(docs, doclen) for _ in range(2)]
        rng = np.random.default_rng(5)
        self.ints = rng.integers(-1 << 40, 1 << 40, docs).astype(np.int64)
        self.dbls = rng.standard_normal(docs)
        self.handles = []

    def rebuild(self):
        for h in self.handles:
            h.close()
        self.handles = []
        for blob, ds in self.blobs:
            g = capi.GpuStringIndex()
            g.build_view(self.ids, blob, ds)
            self.handles.append(g)
        for kind, vals in ((1, self.ints), (2, self.dbls)):
            c = capi.GpuColumn(kind)
            c.add_bulk(self.ids, vals)
            c.build()
            self.handles.append(c)
        for g in self.handles[:2]:
            g.proof_wait()
        return self.handles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--doclen", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shares", default="0.001,0.1")
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = open(a.out, "a") if a.out else None
    db = Fields(a.docs, a.doclen)
    t0 = time.perf_counter()
    db.rebuild()
    emit(fp, bench="rowset_remove_database", docs=a.docs, doclen=a.doclen, fields="2 string + int64 + double",
         build_ms=round((time.perf_counter() - t0) * 1e3, 1))
    rng = np.random.default_rng(11)
    for share in [float(x) for x in a.shares.split(",")]:
        k = max(1, int(round(a.docs * share)))
        gone = np.sort(db.ids[rng.choice(a.docs, size=k, replace=False)])
        zeros = np.zeros(k, dtype=np.int64)
        t_new, t_old, t_old_down, p_new, p_old = [], [], [], [], []
        for _ in range(a.reps):
            for way in ("new", "old"):
                fields = db.rebuild()
                rs = capi.debug_rowset_from_rows(gone, zeros)
                capi.memory_reset_peak()
                base = capi.memory_stats()[0]
                t0 = time.perf_counter()
                if way == "new":
                    rows, res = rs.remove(fields)
                    t_new.append((time.perf_counter() - t0) * 1e3)
                    assert rows == k and all(r["removed"] == k for r in res)
                    p_new.append(capi.memory_stats()[1] - base)
                else:
                    down, _ = rs.rows()
                    t1 = time.perf_counter()
                    got = [f.remove(down) for f in fields]
                    t_old.append((time.perf_counter() - t0) * 1e3)
                    t_old_down.append((t1 - t0) * 1e3)
                    assert all(g == (k, 0) for g in got)
                    p_old.append(capi.memory_stats()[1] - base)
                rs.close()
        emit(fp, bench="rowset_remove", share=share, rows=k, fields=4, reps=a.reps, rowset_remove=stats(t_new), rows_plus_per_field=stats(t_old),
             of_which_download=stats(t_old_down), peak_above_in_use_new=mib(p_new), peak_above_in_use_old=mib(p_old))
    # (c) the union
    fields = db.rebuild()
    lists = [db.ids, db.ids, db.ids, db.ids]   # what a host caller holds: one id list per field
    t_all, t_one, t_host = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rs = capi.rowset_all(fields)
        t_all.append((time.perf_counter() - t0) * 1e3)
        assert rs.size == a.docs
        rs.close()
        t0 = time.perf_counter()
        rs = capi.rowset_all(fields[2:3])
        t_one.append((time.perf_counter() - t0) * 1e3)
        assert rs.size == a.docs
        rs.close()
        t0 = time.perf_counter()
        u = np.unique(np.concatenate(lists))
        rs = capi.debug_rowset_from_rows(u, np.zeros(len(u), dtype=np.int64))
        t_host.append((time.perf_counter() - t0) * 1e3)
        rs.close()
    fields[0].set_option("profile", 1)
    rs = capi.rowset_all(fields)
    kern = {n: {"ms": round(v["ms"], 4), "gbs": round(v["bytes"] / max(v["ms"], 1e-6) / 1e6, 1)} for n, v in rs.profile().items()}
    emit(fp, bench="rowset_all", ids_per_field=a.docs, reps=a.reps, four_fields=stats(t_all), one_field=stats(t_one),
         host_unique_plus_upload=stats(t_host), library_all_ms=round(rs.stat("all_ms"), 3), kernels=kern)
    rs.close()
    for h in db.handles:
        h.close()


if __name__ == "__main__":
    main()
