#!/usr/bin/env python3
"""Measurements behind cdb_insert_objects.

Database: the corpus of tools/bench_rowset_remove.py — two string indexes of --docs documents of --doclen bytes (printable ASCII) plus
an int64 and a double column over the same ids.  For a batch of a share of that many NEW objects (ids above every old one, as
insertion timestamps are; every object holds all four fields) it records, as the caller sees them through the Python binding:
  (a) insert    new: one cdb_insert_objects over the four fields.  old: one cdb_append / cdb_column_append per field through the
                SAME library: that path is unchanged, so it is the comparison, not the code under test.  The two are alternated
                --reps times; the four fields are rebuilt before every timed call (not timed).  Median (min - max).
  (b) memory    the allocator's peak above the in-use level in front of the call, for both ways (the new call holds every field's
                new column beside its old one at the same time).
  (c) id check  the ins_* kernels of one more call with the lead field's option profile on, from the library's own clock, and the
                call's "insert_ms".

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_insert.py [--docs 1048576] [--doclen 256] [--reps 7] [--shares 0.001,0.1] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi, workloads as W  # noqa: E402
from bench_rowset_remove import Fields, emit, mib, stats  # noqa: E402


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
    emit(fp, bench="insert_database", docs=a.docs, doclen=a.doclen, fields="2 string + int64 + double",
         build_ms=round((time.perf_counter() - t0) * 1e3, 1))
    rng = np.random.default_rng(11)
    for share in [float(x) for x in a.shares.split(",")]:
        k = max(1, int(round(a.docs * share)))
        ids = int(db.ids[-1]) + 1 + np.arange(k, dtype=np.int64) * 3
        docs = [W.ascii_corpus(k, a.doclen, seed=777 + j) for j in range(2)]
        ints = rng.integers(-1 << 40, 1 << 40, k).astype(np.int64)
        dbls = rng.standard_normal(k)
        payloads = [docs[0], docs[1], ints, dbls]
        t_new, t_old, p_new, p_old = [], [], [], []

        def one_call(fields):
            return capi.insert_objects(ids, [(f, None, p) for f, p in zip(fields, payloads)])

        for _ in range(a.reps):
            for way in ("new", "old"):
                fields = db.rebuild()
                capi.memory_reset_peak()
                base = capi.memory_stats()[0]
                t0 = time.perf_counter()
                if way == "new":
                    inserted, res = one_call(fields)
                    t_new.append((time.perf_counter() - t0) * 1e3)
                    assert inserted == k and all(r["appended"] == k for r in res)
                    p_new.append(capi.memory_stats()[1] - base)
                else:
                    got = [f.append(ids, *p) if isinstance(p, tuple) else f.append(ids, p) for f, p in zip(fields, payloads)]
                    t_old.append((time.perf_counter() - t0) * 1e3)
                    assert got == [k] * 4
                    p_old.append(capi.memory_stats()[1] - base)
        # (c) one more call with the lead's profile on
        fields = db.rebuild()
        fields[0].set_option("profile", 1)
        fields[0].profile_reset()
        one_call(fields)
        kern = {n: {"ms": round(v["ms"], 4), "launches": v["launches"], "gbs": round(v["bytes"] / max(v["ms"], 1e-6) / 1e6, 1)}
                for n, v in fields[0].profile().items() if n.startswith("ins_")}
        emit(fp, bench="insert_objects", share=share, objects=k, fields=4, reps=a.reps, insert_objects=stats(t_new), per_field_calls=stats(t_old),
             peak_above_in_use_new=mib(p_new), peak_above_in_use_old=mib(p_old),
             library_insert_ms=round(capi.insert_stat(fields[0], "insert_ms"), 3), kernels=kern)
    for h in db.handles:
        h.close()


if __name__ == "__main__":
    main()
