#!/usr/bin/env python3
"""Measurements behind the paged render (cdb_render_rows).

For a page of rows taken from query_ranked it records, as the caller sees them through the Python binding:
  render_rows   one cdb_render_rows call (ids up, rendered strings and spans down);
  parent path   what the same page cost before the paged call existed: cdb_query_spans for the key over ALL matching documents,
                then cdb_shim::render_spans (restated here with bytes slices) over the page's rows from a host copy of the column.
The two are alternated --reps times (7 by default; 3 for pages of 10^6 rows, where the host render alone takes seconds); the line
holds the median and the spread (min, max) of each.  A further profiled call gives the HIP-event time and the achieved bytes/s of
the rnd_* kernels.

Corpora: C1's shape — 2^20 documents of 1 KiB, symbols 0x30.. with Zipf weights so that a 3-byte keyword of the commonest symbols
matches most documents — and valid UTF-8 under reference_compat = 1, where cdb_query_spans scans the whole text.
Keyword lists: one broad 3-byte keyword (UTF-8 corpus, whose ASCII half is uniform: one byte), one selective 8-byte keyword, a list of 16.

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_render.py [--docs 1048576] [--utf8-mib 256] [--reps 7] [--pages 10,100,10000,1000000] [--out FILE]"""
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


def host_render(text, spans, left, right):
    """shim/highlight.h: render_spans"""
    out, at = [], 0
    for b, e in spans:
        out += [text[at:b], left, text[b:e + 1], right]
        at = e + 1
    out.append(text[at:])
    return b"".join(out)


def query_spans_arrays(ix, kws):
    """cdb_query_spans as a C caller sees it: the four result arrays (copied once), no per-span Python objects"""
    import ctypes as C
    blob = np.frombuffer(b"".join(kws), dtype=np.uint8)
    offs = np.zeros(len(kws) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in kws], out=offs[1:])
    r = capi.CdbSpans()
    ix._check(ix._lib.cdb_query_spans(ix._h, capi._ptr(blob), capi._ptr(offs), len(kws), C.byref(r)))
    try:
        nd, ns = int(r.ndocs), int(r.nspans)
        return (capi._array(r.ids, nd, np.int64), capi._array(r.span_ptr, nd + 1, np.uint64).astype(np.int64),
                capi._array(r.begin, ns, np.uint64), capi._array(r.end, ns, np.uint64))
    finally:
        ix._lib.cdb_spans_free(C.byref(r))


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def bench_corpus(fp, name, ix, host_text, ds, ids, lists, pages, reps):
    row_of = {int(i): r for r, i in enumerate(ids)}
    left, right = b"<b>", b"</b>"
    for label, kws in lists:
        ranked = [i for i, _ in ix.query_ranked(kws)]
        for want in pages:
            page = ranked[:want]
            if len(page) < want:   # (fewer matching documents than the page: pad with further documents, as a later page would hold)
                page = (page + [int(i) for i in ids[: want - len(page)]])[:want]
            n_reps = reps if want <= 10000 else min(reps, 3)
            t_new, t_old, t_spans = [], [], []
            same = None
            for _ in range(n_reps):
                t0 = time.perf_counter()
                r = ix.render_rows(page, kws, left, right, raw=True)
                t_new.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                sp_ids, sp_ptr, sp_b, sp_e = query_spans_arrays(ix, kws)
                t1 = time.perf_counter()
                slot = np.searchsorted(sp_ids, page)   # (documents ascend by insertion index and so do these ids)
                texts = []
                for i, k in zip(page, slot.tolist()):
                    d = row_of[i]
                    spans = ()
                    if k < len(sp_ids) and sp_ids[k] == i:
                        spans = zip(sp_b[sp_ptr[k]:sp_ptr[k + 1]].tolist(), sp_e[sp_ptr[k]:sp_ptr[k + 1]].tolist())
                    texts.append(host_render(host_text[int(ds[d]):int(ds[d + 1])], spans, left, right))
                t2 = time.perf_counter()
                t_old.append((t2 - t0) * 1e3)
                t_spans.append((t1 - t0) * 1e3)
                if same is None:   # (under reference_compat on high bytes both are text scans: they agree there too)
                    same = b"".join(texts) == r["text_blob"]
            ix.set_option("profile", 1)
            ix.profile_reset()
            ix.render_rows(page, kws, left, right, raw=True)
            prof = {k: v for k, v in ix.profile().items() if k.startswith("rnd_")}
            ix.set_option("profile", 0)
            kern = {k: {"ms": round(v["ms"], 4), "gbs": round(v["bytes"] / max(v["ms"], 1e-6) / 1e6, 1)} for k, v in prof.items()}
            emit(fp, bench="render", corpus=name, keywords=label, nkw=len(kws), page_rows=len(page), matching_docs=len(ranked),
                 page_bytes=int(ix.stat("render_page_bytes")), spans=int(ix.stat("render_spans")), reps=n_reps, render_rows=stats(t_new),
                 parent_path=stats(t_old), parent_query_spans=stats(t_spans), library_render_ms=round(ix.stat("render_ms"), 3),
                 kernels=kern, outputs_equal=bool(same))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--utf8-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pages", default="10,100,10000,1000000")
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = open(a.out, "a") if a.out else None
    pages = [int(p) for p in a.pages.split(",")]

    def build(text, ds, compat):
        ids = np.arange(len(ds) - 1, dtype=np.int64) * 7 + 1000
        d_ds, d_ids = torch.from_numpy(ds.astype(np.int64)).cuda(), torch.from_numpy(ids).cuda()
        torch.cuda.synchronize()
        ix = capi.GpuStringIndex()
        ix.set_option("reference_compat", compat)
        t0 = time.perf_counter()
        ix.build_resident(text.data_ptr(), d_ds.data_ptr(), d_ids.data_ptr(), len(ids))
        return ix, ids, (time.perf_counter() - t0) * 1e3, (d_ds, d_ids)

    # C1's shape, Zipf symbols
    text = W.zipf_bytes_torch(a.docs * 1024, seed=2)
    ds = W.uniform_docs(a.docs, 1024)
    ix, ids, ms, keep = build(text, ds, 1)
    host = text.cpu().numpy().tobytes()
    rng = np.random.default_rng(7)
    at = [int(x) for x in rng.integers(0, a.docs, 17)]
    lists = [("broad3", [b"012"]), ("selective8", [host[at[0] * 1024 + 100:at[0] * 1024 + 108]]),
             ("list16", [host[d * 1024 + 200:d * 1024 + 200 + 4 + k % 3] for k, d in enumerate(at[1:])])]
    emit(fp, bench="render_corpus", corpus="c1_zipf", docs=a.docs, bytes=len(host), build_ms=round(ms, 1))
    bench_corpus(fp, "c1_zipf", ix, host, ds, ids, lists, pages, a.reps)
    ix.close()
    del text, keep

    # UTF-8 under reference_compat = 1: cdb_query_spans scans the text
    text, ds = W.utf8_bytes_torch(a.utf8_mib << 20)
    ix, ids, ms, keep = build(text, ds, 1)
    host = text.cpu().numpy().tobytes()
    d0 = int(ds[len(ds) // 2])
    lists = [("broad1", [b"e"]), ("selective8", [host[d0:d0 + 8]])]
    emit(fp, bench="render_corpus", corpus="utf8_compat", docs=len(ds) - 1, bytes=len(host), build_ms=round(ms, 1))
    bench_corpus(fp, "utf8_compat", ix, host, ds, ids, lists, [p for p in pages if p <= len(ds) - 1], a.reps)
    ix.close()


if __name__ == "__main__":
    main()
