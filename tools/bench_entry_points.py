"""The host entry points the judged command does not time (it queries through cdb_query_batch_offsets_device): one start = a
64 MiB ASCII corpus built once, then the median of 15 calls each of cdb_query_batch (100 000 patterns), cdb_query_ranked (8
keywords, limit 1000), cdb_query_and (two keys) and the lone-keyword latency inside the library.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi, workloads as W  # noqa: E402


def med(f, reps=15):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def main():
    nd = 262144
    blob, ds = W.ascii_corpus(nd, 256, seed=7)
    ids = np.arange(nd, dtype=np.int64) + 1
    g = capi.GpuStringIndex(device=0)
    g.build_view(ids, blob, ds)
    g.proof_wait()
    pb, po = W.sample_patterns(blob, ds, 100000, 4, 16, seed=3)
    kws = [bytes(pb[int(po[j]):int(po[j + 1])]) for j in range(8)]
    short = [bytes(pb[int(po[j]):int(po[j]) + 2]) for j in range(8, 12)]
    for _ in range(3):
        g.query_batch(pb, po)
    out = {"host_batch_100k_ms": med(lambda: g.query_batch(pb, po)),
           "ranked_8kw_ms": med(lambda: g.query_ranked(short, limit=1000)),
           "and_2keys_ms": med(lambda: capi.query_and([(g, short[:2]), (g, short[2:])], ranked=True, limit=1000)),
           "or_8kw_ms": med(lambda: g.query_or(kws))}
    lat = np.sort(g.query_latency_us(kws, reps=64))
    out["single_query_us_median"] = round(float(lat[len(lat) // 2]), 3)
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
