"""One fixed piece of work for a call-count comparison of two libraries: a build below 2^23 suffixes, one above 2^24, a
force_big_path build in the reference's order on text with bytes >= 0x80, and a query batch.  Run it under `rocprofv3
--kernel-trace --hip-trace --stats` once per library (CDB_LIB_PATH) and compare with tools/build_calls_compare.py."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi, workloads as W  # noqa: E402


def build(corpus, **opts):
    blob, ds = corpus
    g = capi.GpuStringIndex(device=0)
    for k, v in opts.items():
        g.set_option(k, v)
    g.add_bulk(np.arange(len(ds) - 1, dtype=np.int64) + 1, blob, ds)
    g.build()
    for _ in range(600):  # the order proof runs behind the build on a helper thread: let it finish, so that every run makes the same calls
        if g.stat("order_proved") == 1:
            break
        time.sleep(0.05)
    else:
        raise RuntimeError("order proof did not finish")
    return g, blob, ds


def main():
    small, blob, ds = build(W.ascii_corpus(4096, 256, seed=7))           # 2^20 suffixes
    pb, po = W.sample_patterns(blob, ds, 2000, 3, 12, seed=1)
    rp, gi, gc, hits = small.query_batch(pb, po)
    print("small", small.stat("final_depth"), "hits", hits)
    small.close()
    mid, _, _ = build(W.zipf_corpus(20, 1 << 20, seed=3))                # 20 x 2^20 > 2^24 suffixes
    print("mid", mid.stat("final_depth"), mid.stat("bucketed"))
    mid.close()
    big, _, _ = build(W.utf8_corpus(4096, 256, seed=4), force_big_path=1, reference_compat=1)
    print("big", big.stat("final_depth"), big.stat("bucketed"), big.stat("root_folded"))
    big.close()


if __name__ == "__main__":
    main()
