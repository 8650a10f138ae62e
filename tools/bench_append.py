#!/usr/bin/env python3
"""Measurements behind the on-device append (cdb_append).

For a share of fresh documents of the corpus's own distribution it records, as the caller sees them through the Python binding:
  append        one cdb_append call on a built handle (only the new documents are uploaded and sorted);
  parent path   what the same addition cost before the call existed: a FRESH handle built with cdb_build_view over the union of
                old and new documents from host memory (upload + build).  That path is untouched by the append code.
The two are alternated --reps times (at least five); the line holds the median and the spread (min, max) of each.  The handle
the append runs on is rebuilt before every repetition (not timed).  A further profiled call gives the HIP-event time and the
achieved bytes/s of the ap_* kernels.  A last line appends COPIES of existing documents (share --copy-share): every new suffix
has a twin in the old array, so every probe of the rank step that reaches the text compares a whole suffix — the long-common-
prefix case.

Corpus: BASELINE config 1's — 2^20 documents of 1 KiB, printable ASCII, 1 GiB.

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_append.py [--docs 1048576] [--doclen 1024] [--reps 5] [--shares 0.001,0.01,0.1,0.5,1.0]
                                    [--copy-share 0.01] [--out FILE]"""
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


def measure(fp, ix, a, reps, ids, blob, ds, new_ids, new_blob, new_ds, label, share):
    n = int(ds[-1])
    all_ids = np.concatenate([ids, new_ids])
    all_blob = np.concatenate([blob[:n], new_blob[:int(new_ds[-1])]])   # (the union as the caller holds it: not timed)
    all_ds = np.concatenate([ds, new_ds[1:] + np.uint64(n)])
    t_new, t_old, lib_ms = [], [], []
    same = None
    for _ in range(reps):
        ix.build_view(ids, blob, ds)   # (the handle the append runs on: not timed)
        ix.proof_wait()
        t0 = time.perf_counter()
        joined = ix.append(new_ids, new_blob, new_ds)
        t_new.append((time.perf_counter() - t0) * 1e3)
        lib_ms.append(ix.stat("append_ms"))
        assert joined == len(new_ids)
        fresh = capi.GpuStringIndex()
        t0 = time.perf_counter()
        fresh.build_view(all_ids, all_blob, all_ds)
        t_old.append((time.perf_counter() - t0) * 1e3)
        if same is None:
            same = bool(np.array_equal(ix.sa(), fresh.sa()))
        ix.proof_wait()
        fresh.proof_wait()
        fresh.close()
    ix.build_view(ids, blob, ds)
    ix.proof_wait()
    ix.set_option("profile", 1)
    ix.profile_reset()
    ix.append(new_ids, new_blob, new_ds)
    prof = {k: v for k, v in ix.profile().items() if k.startswith("ap_")}
    ix.set_option("profile", 0)
    kern = {k: {"ms": round(v["ms"], 4), "gbs": round(v["bytes"] / max(v["ms"], 1e-6) / 1e6, 1)} for k, v in prof.items()}
    emit(fp, bench="append", corpus="c1_ascii", new_documents=label, share=share, appended_docs=len(new_ids), appended_bytes=int(ix.stat("append_bytes")),
         reps=reps, append=stats(t_new), library_append=stats(lib_ms), parent_build_view=stats(t_old), merge=int(ix.stat("append_merges")),
         keys_kept=int(ix.stat("append_keys_kept")), kernels=kern, arrays_equal=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--doclen", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shares", default="0.001,0.01,0.1,0.5,1.0")
    ap.add_argument("--copy-share", type=float, default=0.01)
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    fp = open(a.out, "a") if a.out else None

    blob, ds = W.ascii_corpus(a.docs, a.doclen)
    ids = np.arange(a.docs, dtype=np.int64) * 7 + 1000
    ix = capi.GpuStringIndex()
    t0 = time.perf_counter()
    ix.build_view(ids, blob, ds)
    emit(fp, bench="append_corpus", corpus="c1_ascii", docs=a.docs, bytes=int(ds[-1]), build_view_ms=round((time.perf_counter() - t0) * 1e3, 1))
    for share in [float(x) for x in a.shares.split(",")]:
        k = max(1, int(round(a.docs * share)))
        new_blob, new_ds = W.ascii_corpus(k, a.doclen, seed=777)   # (fresh documents of the same distribution)
        new_ids = np.arange(k, dtype=np.int64) * 7 + 1000 + 7 * a.docs
        measure(fp, ix, a, reps, ids, blob, ds, new_ids, new_blob, new_ds, "fresh", share)
    if a.copy_share > 0:
        k = max(1, int(round(a.docs * a.copy_share)))
        pick = np.sort(np.random.default_rng(11).choice(a.docs, size=k, replace=False))
        new_blob = np.ascontiguousarray(blob[:int(ds[-1])].reshape(a.docs, a.doclen)[pick]).reshape(-1)
        new_ids = np.arange(k, dtype=np.int64) * 7 + 1000 + 7 * a.docs
        measure(fp, ix, a, reps, ids, blob, ds, new_ids, new_blob, W.uniform_docs(k, a.doclen), "copies", a.copy_share)
    ix.close()


if __name__ == "__main__":
    main()
