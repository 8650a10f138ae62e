#!/usr/bin/env python3
"""Measurements behind the on-device removal (cdb_remove).

For a share of the documents chosen at random it records, as the caller sees them through the Python binding:
  remove        one cdb_remove call on a built handle (ids up, everything else stays on the device);
  parent path   what the same removal cost before the call existed: a FRESH handle built with cdb_build_view over the
                surviving documents from host memory (upload + build).  That path is untouched by the removal code.
The two are alternated --reps times (at least five); the line holds the median and the spread (min, max) of each.  The handle
the removal runs on is rebuilt before every repetition (not timed).  A further profiled call gives the HIP-event time and the
achieved bytes/s of the rm_* kernels.

Corpus: BASELINE config 1's — 2^20 documents of 1 KiB, printable ASCII, 1 GiB.

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_remove.py [--docs 1048576] [--doclen 1024] [--reps 5] [--shares 0.001,0.1,0.5] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--doclen", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shares", default="0.001,0.1,0.5")
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    fp = open(a.out, "a") if a.out else None

    blob, ds = W.ascii_corpus(a.docs, a.doclen)
    ids = np.arange(a.docs, dtype=np.int64) * 7 + 1000
    ix = capi.GpuStringIndex()
    t0 = time.perf_counter()
    ix.build_view(ids, blob, ds)
    emit(fp, bench="remove_corpus", corpus="c1_ascii", docs=a.docs, bytes=int(ds[-1]), build_view_ms=round((time.perf_counter() - t0) * 1e3, 1))
    rng = np.random.default_rng(11)
    text = blob[:int(ds[-1])].reshape(a.docs, a.doclen)
    for share in [float(x) for x in a.shares.split(",")]:
        k = max(1, int(round(a.docs * share)))
        gone = np.sort(rng.choice(a.docs, size=k, replace=False))
        keep = np.ones(a.docs, dtype=bool)
        keep[gone] = False
        kids = ids[keep]
        kblob = np.ascontiguousarray(text[keep]).reshape(-1)   # (the survivors as the caller holds them: not timed)
        kds = W.uniform_docs(len(kids), a.doclen)
        gone_ids = ids[gone]
        t_new, t_old, lib_ms = [], [], []
        same = None
        for _ in range(reps):
            ix.build_view(ids, blob, ds)   # (the handle the removal runs on: not timed)
            ix.proof_wait()
            t0 = time.perf_counter()
            removed, missing = ix.remove(gone_ids)
            t_new.append((time.perf_counter() - t0) * 1e3)
            lib_ms.append(ix.stat("remove_ms"))
            assert (removed, missing) == (k, 0)
            fresh = capi.GpuStringIndex()
            t0 = time.perf_counter()
            fresh.build_view(kids, kblob, kds)
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
        ix.remove(gone_ids)
        prof = {n: v for n, v in ix.profile().items() if n.startswith("rm_")}
        ix.set_option("profile", 0)
        kern = {n: {"ms": round(v["ms"], 4), "gbs": round(v["bytes"] / max(v["ms"], 1e-6) / 1e6, 1)} for n, v in prof.items()}
        emit(fp, bench="remove", corpus="c1_ascii", share=share, removed_docs=k, removed_bytes=int(ix.stat("remove_bytes")), reps=reps,
             remove=stats(t_new), library_remove=stats(lib_ms), parent_build_view=stats(t_old), compaction=int(ix.stat("remove_compactions")),
             kernels=kern, arrays_equal=same)
    ix.close()


if __name__ == "__main__":
    main()
