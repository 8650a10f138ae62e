#!/usr/bin/env python3
"""Measurements behind remove / append / cluster on a sharded string column (cdb_shards_remove,
cdb_shards_append, cdb_shards_cluster).

One size that a single MI355X holds as four co-resident shards (device slots 0,0,0,0: the shards exchange through device copies,
so this says nothing about several GPUs).  For each operation it records the wall time of the call as the caller sees it through
the Python binding, and beside it what the same change cost before the call existed: a fresh cdb_shards_build of the same FINAL
column (the column is staged with cdb_shards_add_bulk first; the staging is not timed — only the build is).  That rebuild is
existing code.  The two are alternated --reps times (at least five); every line holds the median and the spread (min, max).  The
set the call runs on is rebuilt before every repetition and its order proofs are awaited (not timed).  shard_ms is the largest
"remove_ms" / "append_ms" any shard reports for the call (wall time inside that shard, under its lock).  Every writer is measured
twice: on a set built as the shim builds it (cdb_shards_build_views: nothing is staged in the handle, "staged": false) and on one
built with cdb_shards_add_bulk + cdb_shards_build, whose host staging copy of the whole column the call has to release
("staged": true).
  remove         a share of the documents, spread evenly over all shards;
  append_last    a share of fresh documents that joins the last shard (every device slot is in use);
  append_grow    the same documents opening a fifth shard (max_shard_bytes = a quarter of the column, five slots);
  cluster        every fourth row grouped, with and without the strings, against cdb_cluster on ONE index over the same column.
The tool reports; it gates nothing.

Corpus: --docs documents of --doclen bytes, printable ASCII (BASELINE config 1's distribution).

Every line of output is one JSON object; --out also appends them to a file.
usage: python tools/bench_shards_maintain.py [--docs 1048576] [--doclen 1024] [--reps 5] [--share 0.01] [--out FILE]"""
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


def sharded(slots, ids, blob, ds, docs=None, **opts):
    """docs (a list of bytes): built from views, nothing staged; else staged with add_bulk and built"""
    sh = capi.GpuShards([0] * slots)
    for k, v in opts.items():
        sh.set_option(k, v)
    if docs is not None:
        sh.build_views(ids, docs)
    else:
        sh.add_bulk(ids, blob, ds)
        sh.build()
    return sh


def settle(sh):
    for i in range(sh.count):
        sh.shard(i).proof_wait()


def timed_rebuild(slots, ids, blob, ds, **opts):
    """a fresh cdb_shards_build over the final column; the staging copy is made first and not timed"""
    sh = capi.GpuShards([0] * slots)
    for k, v in opts.items():
        sh.set_option(k, v)
    sh.add_bulk(ids, blob, ds)
    t0 = time.perf_counter()
    sh.build()
    ms = (time.perf_counter() - t0) * 1e3
    return sh, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--doclen", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--out")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    fp = open(a.out, "a") if a.out else None
    D, L = a.docs, a.doclen
    blob, ds = W.ascii_corpus(D, L)
    ids = np.arange(D, dtype=np.int64) * 7 + 1000
    total = int(ds[-1])
    k = max(1, int(round(D * a.share)))
    common = dict(bench="shards_maintain", corpus="c1_ascii", docs=D, bytes=total, shards=4, share=a.share, reps=reps)
    raw = blob[:total].tobytes()
    docs = [raw[i * L:(i + 1) * L] for i in range(D)]

    # ---- remove: every (D / k)-th document, so every shard loses its share
    gone_at = np.arange(k, dtype=np.int64) * (D // k)
    keep = np.ones(D, dtype=bool)
    keep[gone_at] = False
    kept_blob = np.ascontiguousarray(blob[:total].reshape(D, L)[keep]).reshape(-1)
    kept_ids, kept_ds = ids[keep], W.uniform_docs(D - k, L)
    for staged in (False, True):
        t_new, t_old, t_lib, same = [], [], [], None
        for _ in range(reps):
            sh = sharded(4, ids, blob, ds, None if staged else docs, use_all_devices=1)
            settle(sh)
            t0 = time.perf_counter()
            removed, missing = sh.remove(ids[gone_at])
            t_new.append((time.perf_counter() - t0) * 1e3)
            t_lib.append(max(sh.shard(i).stat("remove_ms") for i in range(4)))
            assert (removed, missing) == (k, 0)
            fresh, ms = timed_rebuild(4, kept_ids, kept_blob, kept_ds, use_all_devices=1)
            t_old.append(ms)
            if same is None:
                same = sh.query(b"the") == fresh.query(b"the") and sh.query(b"qz") == fresh.query(b"qz")
            compactions = [int(sh.shard(i).stat("remove_compactions")) for i in range(4)]
            settle(sh)
            settle(fresh)
            sh.close()
            fresh.close()
        emit(fp, **common, op="remove", staged=staged, docs_changed=k, call=stats(t_new), shard_ms=stats(t_lib), rebuild=stats(t_old), compactions=compactions, answers_equal=bool(same))

    # ---- append: fresh documents of the same distribution
    new_blob, new_ds = W.ascii_corpus(k, L, seed=777)
    new_ids = np.arange(k, dtype=np.int64) * 7 + 1000 + 7 * D
    all_ids = np.concatenate([ids, new_ids])
    all_blob = np.concatenate([blob[:total], new_blob[:int(new_ds[-1])]])
    all_ds = W.uniform_docs(D + k, L)
    for op, slots, opts, want, staged in (("append_last", 4, dict(use_all_devices=1), 4, False), ("append_last", 4, dict(use_all_devices=1), 4, True),
                                          ("append_grow", 5, dict(max_shard_bytes=total // 4), 5, False)):
        t_new, t_old, t_lib, same = [], [], [], None
        for _ in range(reps):
            sh = sharded(slots, ids, blob, ds, None if staged else docs, **opts)
            assert sh.count == 4
            settle(sh)
            t0 = time.perf_counter()
            joined = sh.append(new_ids, new_blob, new_ds)
            t_new.append((time.perf_counter() - t0) * 1e3)
            t_lib.append(max(sh.shard(i).stat("append_ms") for i in range(4)))   # (append_grow: a build on a new shard, not an append)
            assert joined == k and sh.count == want
            fresh, ms = timed_rebuild(slots, all_ids, all_blob, all_ds, **opts)
            t_old.append(ms)
            if same is None:
                same = sh.query(b"the") == fresh.query(b"the") and sh.query(b"qz") == fresh.query(b"qz")
            settle(sh)
            settle(fresh)
            sh.close()
            fresh.close()
        emit(fp, **common, op=op, staged=staged, docs_changed=k, shards_after=want, call=stats(t_new), shard_ms=stats(t_lib), rebuild=stats(t_old), answers_equal=bool(same))

    # ---- cluster: every fourth row
    sh = sharded(4, ids, blob, ds, use_all_devices=1)
    one = capi.GpuStringIndex()
    one.build_view(ids, blob, ds)
    rows = ids[::4]
    for with_values in (True, False):
        sh.cluster(rows, with_values=with_values)   # (the class tables are made at the first call: not timed)
        one.cluster(rows, with_values=with_values)
        t_sh, t_one = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            a_ = sh.cluster(rows, with_values=with_values)
            t_sh.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            b_ = one.cluster(rows, with_values=with_values)
            t_one.append((time.perf_counter() - t0) * 1e3)
        same = a_[0] == b_[0] and np.array_equal(a_[1], b_[1]) and np.array_equal(a_[2], b_[2]) and a_[3] == b_[3]
        emit(fp, **common, op="cluster", rows=len(rows), with_values=with_values, groups=len(a_[1]), call=stats(t_sh), single_index=stats(t_one),
             answers_equal=bool(same))
    sh.close()
    one.close()


if __name__ == "__main__":
    main()
