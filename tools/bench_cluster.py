#!/usr/bin/env python3
"""Measurements behind `cluster` on the device (cdb_column_cluster / cdb_cluster).

  column sweep   both paths of cdb_column_cluster forced (debug_cluster_path) over a range of result-set sizes: the table the
                 sparse / dense constant of cluster.hip is derived from.  Per size: caller's wall time (median of --reps calls through
                 the Python binding), the library's own wall clock (stat cluster_ms: upload .. results on the host), the summed
                 HIP-event time of its kernels (profile = 1, a separate call), and the host loop it replaces on the same rows.
  string column  the one-off preparation (stat cluster_prepare_ms) beside the column's build time, event-timed bytes/s of the
                 compaction pass, and the per-call time at a few result sizes.

The host loop is database.cpp:442-460 restated with numpy (labelled "numpy"): id -> row by binary search over the sorted ids (the
reference's unordered_map lookup), then np.unique over the values — a vectorised stand-in that is FASTER than the reference's
per-row std::map<std::string> insertions, so the comparison errs against the device.

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_cluster.py [--rows 10000000] [--distinct 1000] [--string-mib 256] [--big-gib 0] [--distinct-mib 0] [--reps 5]
                                     [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi  # noqa: E402

PEAK_TBS = 8.0  # MI355X HBM3E


def emit(fp, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if fp:
        fp.write(line + "\n")
        fp.flush()


def median_wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def event_ms(obj, fn):
    """summed HIP-event time of the kernels one call launches"""
    obj.set_option("profile", 1)
    before = {k: v["ms"] for k, v in obj.profile().items()}
    fn()
    after = obj.profile()
    obj.set_option("profile", 0)
    return {k: round(v["ms"] - before.get(k, 0.0), 4) for k, v in after.items() if v["ms"] - before.get(k, 0.0) > 0}


def column_sweep(fp, n, distinct, reps):
    rng = np.random.default_rng(1)
    ids = np.arange(n, dtype=np.int64) * 3 + 1_700_000_000_000  # timestamps
    vals = rng.integers(0, distinct, n).astype(np.int64) * 7919
    col = capi.GpuColumn(1, device=0)
    col.add_bulk(ids, vals)
    col.build()
    emit(fp, what="column", rows=n, distinct=distinct, build_ms=round(col.stat("build_ms"), 3))
    for frac in (0.0001, 0.001, 0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.75, 0.9, 1.0):
        k = max(1, int(n * frac))
        rows = np.sort(rng.choice(n, k, replace=False)) if k < n else np.arange(n)
        rows = ids[rows]  # ascending by id: what filter() returns unranked
        rec = dict(what="column_cluster", rows=n, selected=k, share=frac)
        for name, path in (("sparse", 1), ("dense", 2)):
            col.set_option("debug_cluster_path", path)
            col.cluster(rows)  # warm: work spaces, run starts
            rec[name + "_wall_ms"] = round(median_wall_ms(lambda: col.cluster(rows), reps), 4)
            rec[name + "_lib_ms"] = round(col.stat("cluster_ms"), 4)
            ev = event_ms(col, lambda: col.cluster(rows))
            rec[name + "_event_ms"] = round(sum(ev.values()), 4)
            rec[name + "_kernels"] = ev
        col.set_option("debug_cluster_path", 0)

        def host_loop():
            r = np.searchsorted(ids, rows)
            return np.unique(vals[r], return_counts=True)
        rec["host_numpy_ms"] = round(median_wall_ms(host_loop, max(1, reps // 2)), 4)
        emit(fp, **rec)
    col.close()


def string_column(fp, total_bytes, reps, label):
    dl = 1024
    nd = total_bytes // dl
    npool = max(16, min(10 ** 4, nd // 8))
    rng = np.random.default_rng(2)
    pool = rng.integers(0x61, 0x7B, (npool, dl), dtype=np.uint8)
    pick = rng.integers(0, npool, nd)
    ids = np.arange(nd, dtype=np.int64) * 3 + 1_700_000_000_000
    ds = np.arange(nd + 1, dtype=np.uint64) * dl
    g = capi.GpuStringIndex(device=0)
    step = 1 << 16
    blob = np.empty(nd * dl, dtype=np.uint8)
    for a in range(0, nd, step):
        blob[a * dl:(a + step) * dl] = pool[pick[a:a + step]].reshape(-1)
    g.build_view(ids, blob, ds)
    del blob
    g.proof_wait()
    # the kernels' code object is loaded at its first launch: a throw-away index takes that cost, not the brackets below
    w = capi.GpuStringIndex(device=0)
    w.add_bulk(np.arange(4, dtype=np.int64), np.frombuffer(b"abcdabcd", dtype=np.uint8), np.array([0, 2, 4, 6, 8], dtype=np.uint64))
    w.build()
    w.cluster(np.arange(4, dtype=np.int64))
    w.close()
    g.set_option("profile", 1)
    t0 = time.perf_counter()
    g.cluster(ids[:1], with_values=False)  # the first call makes the class table
    first_ms = (time.perf_counter() - t0) * 1e3
    prof = g.profile()
    g.set_option("profile", 0)
    zero = {"ms": 0.0, "bytes": 0}
    cnt, wr = prof.get("clu_compact_count", zero), prof.get("clu_compact_write", zero)   # kernels only, one bracket each

    def rate(r):
        return round(r["bytes"] / r["ms"] / 1e9, 3) if r["ms"] else None
    emit(fp, what="string_prepare", label=label, text_bytes=nd * dl, documents=nd, classes=int(g.stat("cluster_classes")),
         build_ms=round(g.stat("build_ms"), 3), prepare_ms=round(g.stat("cluster_prepare_ms"), 3), first_call_wall_ms=round(first_ms, 3),
         table_bytes=int(g.stat("cluster_table_bytes")), sa_bytes_per_entry=g.stat("sa_bytes_per_entry"),
         compact_count_event_ms=round(cnt["ms"], 4), compact_count_bytes=int(cnt["bytes"]), compact_count_tb_per_s=rate(cnt),
         compact_write_event_ms=round(wr["ms"], 4), compact_write_bytes=int(wr["bytes"]), compact_write_tb_per_s=rate(wr),
         peak_tb_per_s=PEAK_TBS,
         prepare_kernels={k: round(v["ms"], 4) for k, v in prof.items() if k.startswith("clu_")})
    for k in (100, 10_000, nd // 10, nd):
        k = min(k, nd)
        rows = ids[np.sort(rng.choice(nd, k, replace=False))]
        g.cluster(rows, with_values=False)
        rec = dict(what="string_cluster", label=label, documents=nd, selected=k)
        rec["wall_ms"] = round(median_wall_ms(lambda: g.cluster(rows, with_values=False), reps), 4)
        rec["lib_ms"] = round(g.stat("cluster_ms"), 4)
        rec["with_values_wall_ms"] = round(median_wall_ms(lambda: g.cluster(rows, with_values=True), max(1, reps // 2)), 4)
        ev = event_ms(g, lambda: g.cluster(rows, with_values=False))
        rec["event_ms"] = round(sum(ev.values()), 4)

        def host_loop():
            r = np.searchsorted(ids, rows)
            return np.unique(pick[r], return_counts=True)  # (the document's pool number stands in for its text: no string compares)
        rec["host_numpy_ms"] = round(median_wall_ms(host_loop, max(1, reps // 2)), 4)
        emit(fp, **rec)
    g.close()
    capi.load_library().cdb_release_cached_memory()


def string_reference_order(fp, total_bytes):
    """The costly case of the preparation: text with bytes on both sides of 0x80 under reference_compat (the array is in the
    reference's order) and every document distinct — one document per class, i.e. the whole column, is downloaded and sorted on
    the host while the handle's lock is held."""
    dl = 256
    nd = total_bytes // dl
    rng = np.random.default_rng(3)
    blob = rng.integers(0x70, 0x91, nd * dl, dtype=np.uint8)
    ids = np.arange(nd, dtype=np.int64)
    ds = np.arange(nd + 1, dtype=np.uint64) * dl
    g = capi.GpuStringIndex(device=0)
    g.build_view(ids, blob, ds)
    g.proof_wait()
    t0 = time.perf_counter()
    g.cluster(ids[:1], with_values=False)
    first_ms = (time.perf_counter() - t0) * 1e3
    emit(fp, what="string_prepare_reference_order", text_bytes=nd * dl, documents=nd, classes=int(g.stat("cluster_classes")),
         resorted=int(g.stat("cluster_resorted")), compat_rotations=int(g.stat("compat_rotations")), build_ms=round(g.stat("build_ms"), 3),
         prepare_ms=round(g.stat("cluster_prepare_ms"), 3), first_call_wall_ms=round(first_ms, 3))
    g.close()
    capi.load_library().cdb_release_cached_memory()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--string-mib", type=int, default=256)
    ap.add_argument("--big-gib", type=float, default=0.0, help="also a multi-GiB string column of this size (0 = skip)")
    ap.add_argument("--distinct-mib", type=int, default=0, help="also a column of distinct documents in the reference's order (0 = skip)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = open(a.out, "a") if a.out else None
    if a.rows:
        column_sweep(fp, a.rows, a.distinct, a.reps)
    if a.string_mib:
        string_column(fp, a.string_mib << 20, a.reps, f"{a.string_mib} MiB")
    if a.big_gib:
        string_column(fp, int(a.big_gib * (1 << 30)), a.reps, f"{a.big_gib:g} GiB")
    if a.distinct_mib:
        string_reference_order(fp, a.distinct_mib << 20)


if __name__ == "__main__":
    main()
