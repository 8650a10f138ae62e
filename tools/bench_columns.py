#!/usr/bin/env python3
"""Numeric / bool columns on one MI355X (cdb_column_*): build, query_any by selectivity, the dense / sparse crossover, an AND of a
selective substring key with a broad integer range, and per-kernel bandwidth.  Writes JSON under --out.

legs (--legs, comma separated; default all but kernels):
  build      build time of an int64 and a double column of --rows rows (ids ascending = insertion timestamps; random values)
  select     query_any at selectivities 1e-6 .. 90 % on the int64 column: automatic path, and both paths forced
             (option debug_query_path) — the crossover of DESIGN.md §7.1
  and        C1-style corpus (2^20 x 1 KiB ASCII documents) with an int64 column over the same ids: a selective 3-byte
             substring key AND a 50 % range, (a) through the column (cdb_query_and_columns) and (b) the route before columns:
             the range answered in (value, id) order on the host, sorted by id with numpy, uploaded as host rows (cdb_query_and)
  and_large  the same comparison at --rows rows: 1000 selective host rows AND a 50 % range, as a column key or as host rows
  kernels    the build and the query legs once more with the library's own event timing (option profile): per kernel family,
             algorithmic bytes over time against 8 TB/s.  With --rocprof the same leg runs in a child process under
             `rocprofv3 --kernel-trace --stats` and the kernel statistics land under --out/rocprof.
usage: python tools/bench_columns.py --out DIR [--rows N] [--legs build,select,and,and_large] [--reps R] [--rocprof]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes/s (MI355X_MICROARCH.md)
SELECTIVITIES = [1e-6, 1e-3, 1e-2, 0.1, 0.5, 0.9]
VMAX = 10 ** 9


def _sync():
    import torch
    torch.cuda.synchronize()


def _column(kind, ids, vals):
    from coffeedb_amd import capi
    c = capi.GpuColumn(kind, device=0)
    c.add_bulk(ids, vals)
    t0 = time.perf_counter()
    c.build()
    return c, (time.perf_counter() - t0) * 1e3


def leg_build(args, out):
    rng = np.random.default_rng(1)
    n = args.rows
    ids = np.arange(n, dtype=np.int64) + 1_700_000_000_000
    res = {}
    for kind, vals in (("int64", rng.integers(0, VMAX, n, dtype=np.int64)), ("double", rng.standard_normal(n))):
        times, dev = [], []
        for _ in range(args.reps):
            c, ms = _column(kind, ids, vals)
            times.append(ms)
            dev.append(c.stat("build_ms"))
            c.close()
        # a second layout: ids not ascending (the id sort runs)
        perm_ids = ids[rng.permutation(n)] if kind == "int64" else None
        res[kind] = {"rows": n, "build_ms_wall": times, "build_ms_library": dev, "build_ms_median": float(np.median(times))}
        if perm_ids is not None:
            c, ms = _column(kind, perm_ids, vals)
            res[kind]["shuffled_ids_build_ms"] = ms
            res[kind]["shuffled_ids_id_sort_skipped"] = c.stat("id_sort_skipped")
            c.close()
    out["build"] = res


def _timed(fn, reps):
    ts = []
    r = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


def leg_select(args, out):
    rng = np.random.default_rng(2)
    n = args.rows
    ids = np.arange(n, dtype=np.int64) + 1_700_000_000_000
    vals = rng.integers(0, VMAX, n, dtype=np.int64)
    col, _ = _column("int64", ids, vals)
    rows = []
    for s in SELECTIVITIES:
        hi = max(0, int(VMAX * s) - 1)
        rng_s = [f"[0,{hi}]"]
        entry = {"selectivity": s, "range": rng_s[0]}
        for path, name in ((0, "auto"), (1, "sparse"), (2, "dense")):
            col.set_option("debug_query_path", path)
            sp0, dn0 = col.stat("sparse_queries"), col.stat("dense_queries")
            dev = []

            def q():
                r = col.query_any(rng_s)
                dev.append(col.stat("last_union_ms"))
                return r
            r, ts = _timed(q, args.reps)
            entry[name] = {"ms": ts, "ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "rows": int(len(r)),
                           "device_ms": dev, "device_ms_median": float(np.median(dev))}
            if path == 0:
                entry["auto_path"] = "sparse" if col.stat("sparse_queries") > sp0 else ("dense" if col.stat("dense_queries") > dn0 else "none")
        entry["k_over_n"] = col.stat("last_k") / n
        rows.append(entry)
    col.set_option("debug_query_path", 0)
    # crossover: the smallest measured selectivity at which the forced dense path beats the forced sparse one
    cross = [e["selectivity"] for e in rows if e["dense"]["device_ms_median"] < e["sparse"]["device_ms_median"]]
    out["select"] = {"rows": n, "by_selectivity": rows, "dense_wins_from_selectivity": min(cross) if cross else None}
    # finer sweep, up to where the paths cross
    fine = []
    for s in (0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95):
        hi = int(VMAX * s) - 1
        e = {"selectivity": s}
        for path, name in ((1, "sparse"), (2, "dense")):
            col.set_option("debug_query_path", path)
            dev = []
            for _ in range(args.reps):
                col.query_any([f"[0,{hi}]"])
                dev.append(col.stat("last_union_ms"))
            e[name + "_device_ms_median"] = float(np.median(dev))
            e[name + "_device_ms"] = dev
        fine.append(e)
    col.set_option("debug_query_path", 0)
    out["select"]["crossover_sweep"] = fine
    col.close()


def leg_and(args, out):
    import torch
    from coffeedb_amd import capi, workloads as W
    ndocs, doclen = 1 << 20, 1024
    text = W.random_bytes_torch(ndocs * doclen, seed=12345, device="cuda")
    _sync()
    ds = np.arange(ndocs + 1, dtype=np.uint64) * doclen
    ids = np.arange(ndocs, dtype=np.int64) * 3 + 1_700_000_000_000
    g = capi.GpuStringIndex(device=0)
    g.build_device(text.data_ptr(), ds, ids)
    kw = bytes(text[1000:1003].cpu().numpy().tobytes())  # a 3-byte substring of the corpus: ~1/95^3 of the positions
    rng = np.random.default_rng(3)
    vals = rng.integers(0, VMAX, ndocs, dtype=np.int64)
    col, _ = _column("int64", ids, vals)
    rng_s = f"[0,{VMAX // 2 - 1}]"  # 50 %
    # host route: (value, id)-ordered rows as the CPU integer_index returns them, sorted by id, handed over as host rows
    order = np.lexsort((ids, vals))
    sv, si = vals[order], ids[order]

    def host_route():
        a, b = np.searchsorted(sv, 0, "left"), np.searchsorted(sv, VMAX // 2 - 1, "right")
        rows_ids = np.sort(si[a:b])
        return capi.query_and([(g, [kw]), (None, list(zip(rows_ids.tolist(), [0] * len(rows_ids))))])

    def host_route_arrays():  # the same without the Python list: the numpy sort + cdb_query_and only
        import ctypes as C
        a, b = np.searchsorted(sv, 0, "left"), np.searchsorted(sv, VMAX // 2 - 1, "right")
        rows_ids = np.ascontiguousarray(np.sort(si[a:b]))
        zeros = np.zeros(len(rows_ids), dtype=np.int64)
        lib = capi.load_library()
        blob = np.frombuffer(kw, dtype=np.uint8)
        offs = np.array([0, len(kw)], dtype=np.uint64)
        keys = (capi.CdbKeyQuery * 2)()
        keys[0].index = g._h
        keys[0].blob = blob.ctypes.data
        keys[0].offsets = offs.ctypes.data
        keys[0].nkw = 1
        keys[1].ids = rows_ids.ctypes.data
        keys[1].counts = zeros.ctypes.data
        keys[1].nrows = len(rows_ids)
        oi, oc, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        assert lib.cdb_query_and(keys, 2, 0, 0, 0, 0, C.byref(oi), C.byref(oc), C.byref(n)) == 0
        res = [(oi[i], oc[i]) for i in range(n.value)]
        lib.cdb_free(oi)
        lib.cdb_free(oc)
        return res

    def column_route():
        return capi.query_and([(g, [kw]), (col, [rng_s])])

    p0 = col.stat("probe_filters")
    ref = host_route_arrays()
    got = column_route()
    assert got == ref, "column AND differs from the host-rows AND"
    res = {"corpus_GiB": ndocs * doclen / 2 ** 30, "keyword": kw.decode(errors="replace"), "range": rng_s, "result_rows": len(got),
           "string_key_rows": len(g.query_or([kw])), "probe_path": col.stat("probe_filters") > p0}
    tc, th, tl = [], [], []
    for _ in range(args.reps):  # alternated
        _, t = _timed(column_route, 1)
        tc += t
        _, t = _timed(host_route_arrays, 1)
        th += t
    for _ in range(max(1, args.reps // 3)):
        _, t = _timed(host_route, 1)
        tl += t
    res["column_ms"] = tc
    res["host_rows_ms"] = th
    res["host_rows_python_list_ms"] = tl
    for k in ("column_ms", "host_rows_ms"):
        res[k + "_median"] = float(np.median(res[k]))
        res[k + "_spread"] = [float(np.min(res[k])), float(np.max(res[k]))]
    res["speedup_median"] = res["host_rows_ms_median"] / res["column_ms_median"]
    out["and"] = res
    col.close()
    g.close()
    del text
    torch.cuda.empty_cache()


def leg_and_large(args, out):
    """The table size of the issue: --rows rows, a selective key of 1000 host rows AND a 50 % range.  Host route: the range's
    rows in (value, id) order (what integer_index::query returns), np.sort by id, uploaded as host rows (cdb_query_and needs a
    string key, so cdb_query_and_columns carries both routes: the range as host rows, or as the column key)."""
    import ctypes as C
    from coffeedb_amd import capi
    rng = np.random.default_rng(5)
    n = args.rows
    ids = np.arange(n, dtype=np.int64) + 1_700_000_000_000
    vals = rng.integers(0, VMAX, n, dtype=np.int64)
    col, _ = _column("int64", ids, vals)
    sel = np.sort(rng.choice(ids, 1000, replace=False))
    order = np.lexsort((ids, vals))
    sv, si = vals[order], ids[order]
    del order
    lib = capi.load_library()
    zeros_sel = np.zeros(len(sel), dtype=np.int64)
    rng_s = f"[0,{VMAX // 2 - 1}]"

    def run(host_rows):
        keys = (capi.CdbKeyQuery * 2)()
        keys[0].ids = sel.ctypes.data
        keys[0].counts = zeros_sel.ctypes.data
        keys[0].nrows = len(sel)
        nk = 1
        keep = []
        cols = (capi.CdbColumnKey * 1)()
        if host_rows:
            a, b = np.searchsorted(sv, 0, "left"), np.searchsorted(sv, VMAX // 2 - 1, "right")
            rows_ids = np.ascontiguousarray(np.sort(si[a:b]))
            z = np.zeros(len(rows_ids), dtype=np.int64)
            keep += [rows_ids, z]
            keys[1].ids = rows_ids.ctypes.data
            keys[1].counts = z.ctypes.data
            keys[1].nrows = len(rows_ids)
            nk = 2
        # (host rows alone have no device to run on: the host route carries the column with its full range, which adds a probe
        #  of the <= 1000 merged rows and nothing else)
        blob, offs = capi.GpuColumn._pack(["[-inf,inf]"] if host_rows else [rng_s])
        keep += [blob, offs]
        cols[0].column = col._h
        cols[0].blob = blob.ctypes.data
        cols[0].offsets = offs.ctypes.data
        cols[0].nranges = 1
        oi, oc, nr = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
        assert lib.cdb_query_and_columns(keys, nk, cols, 1, 0, 0, 0, 0, C.byref(oi), C.byref(oc), C.byref(nr)) == 0
        res = np.ctypeslib.as_array(oi, shape=(nr.value,)).copy() if nr.value else np.empty(0, np.int64)
        lib.cdb_free(oi)
        lib.cdb_free(oc)
        return res

    a0 = run(True)
    b0 = run(False)
    assert np.array_equal(a0, b0)
    tc, th = [], []
    for _ in range(max(3, args.reps // 2)):
        tc += _timed(lambda: run(False), 1)[1]
        th += _timed(lambda: run(True), 1)[1]
    out["and_large"] = {"rows": n, "selective_key_rows": len(sel), "range": rng_s, "result_rows": int(len(b0)),
                        "probe_filters": col.stat("probe_filters"), "column_ms": tc, "host_rows_ms": th,
                        "column_ms_median": float(np.median(tc)), "host_rows_ms_median": float(np.median(th)),
                        "column_ms_spread": [float(np.min(tc)), float(np.max(tc))], "host_rows_ms_spread": [float(np.min(th)), float(np.max(th))]}
    col.close()


def leg_kernels(args, out):
    rng = np.random.default_rng(4)
    n = args.rows
    ids = np.arange(n, dtype=np.int64) + 1_700_000_000_000
    res = {}
    for kind, vals, shuffle in (("int64", rng.integers(0, VMAX, n, dtype=np.int64), False),
                                ("int64_shuffled_ids", rng.integers(0, VMAX, n, dtype=np.int64), True),
                                ("double", rng.standard_normal(n), False)):
        from coffeedb_amd import capi
        c = capi.GpuColumn("double" if kind == "double" else "int64", device=0)
        c.set_option("profile", 1)
        c.add_bulk(ids[rng.permutation(n)] if shuffle else ids, vals)
        c.build()
        if kind == "int64":
            for s in (1e-3, 1e-2, 0.5):
                c.query_any([f"[0,{int(VMAX * s) - 1}]"])
        prof = c.profile()
        for k, v in prof.items():
            v["GB_per_s"] = v["bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else None
            v["share_of_hbm_peak"] = v["bytes"] / (v["ms"] * 1e-3) / HBM_PEAK if v["ms"] > 0 else None
        res[kind] = prof
        c.close()
    out["kernels_event_timed"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--legs", default="build,select,and,and_large")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true", help="run the kernels leg in a child under rocprofv3 --kernel-trace --stats")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.rocprof:
        d = os.path.join(args.out, "rocprof")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "columns", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--out", os.path.join(args.out, "under_rocprof"), "--rows", str(args.rows),
               "--legs", "kernels", "--reps", "1"]
        r = subprocess.run(cmd, timeout=900)
        sys.exit(r.returncode)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_columns: no GPU (there is no CPU path)")
    out = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "reps": args.reps}
    legs = {"build": leg_build, "select": leg_select, "and": leg_and, "and_large": leg_and_large, "kernels": leg_kernels}
    for name in args.legs.split(","):
        t0 = time.perf_counter()
        legs[name](args, out)
        out.setdefault("leg_seconds", {})[name] = time.perf_counter() - t0
        with open(os.path.join(args.out, "bench_columns.json"), "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k in ("device", "rows", "leg_seconds")}))


if __name__ == "__main__":
    main()
