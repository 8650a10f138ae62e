"""One fixed piece of work on a sharded column for a call-count comparison of two libraries (tools/build_calls_compare.py is the
comparer; tools/build_calls_script.py is its counterpart for the build): over three co-resident shards on one device a sharded build,
a build from views, a save and a load, a batch merged on the host and on the devices, a remove, an append that opens a shard, and
one merge and one counts-only merge over a three-rank group.  Run it under `rocprofv3 --kernel-trace --hip-trace --stats` once per
library (CDB_LIB_PATH); every order proof is awaited, so that every run makes the same calls."""
import os
import sys
import tempfile
import threading

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi, workloads as W  # noqa: E402


def settle(sh):
    for i in range(sh.count):
        sh.shard(i).proof_wait()


def collective(fn, world):
    out = [None] * world
    th = [threading.Thread(target=lambda r=r: out.__setitem__(r, fn(r))) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    return out


def main():
    nd = 3000
    blob, ds = W.ragged_corpus(nd, 120, seed=5, lo=0x61, hi=0x64)
    ids = np.arange(nd, dtype=np.int64) * 3 + 1
    pb, po = W.sample_patterns(blob, ds, 500, 1, 6, seed=2)
    sh = capi.GpuShards([0, 0, 0])
    sh.set_option("use_all_devices", 1)
    sh.add_bulk(ids, blob, ds)
    sh.build()
    settle(sh)
    for dm in (0, 1):
        sh.set_option("device_merge", dm)
        print("batch device_merge", dm, "hits", sh.query_batch(pb, po)[3])
    print("remove", sh.remove(ids[::50]))
    settle(sh)
    with tempfile.TemporaryDirectory() as tmp:
        sh.save(os.path.join(tmp, "col"))
        sl = capi.GpuShards([0, 0, 0])
        sl.load(os.path.join(tmp, "col"))
        settle(sl)
        print("loaded", sl.count, "hits", sl.query_batch(pb, po)[3])
        sl.close()
    sh.close()
    sv = capi.GpuShards([0, 0, 0])                                   # two shards by size, one idle slot
    sv.set_option("max_shard_bytes", int(ds[-1]) // 2 + 200)
    sv.build_views(ids, [bytes(blob[int(ds[d]):int(ds[d + 1])]) for d in range(nd)])
    settle(sv)
    assert sv.count == 2
    nb, nds = W.ragged_corpus(1500, 120, seed=6, lo=0x61, hi=0x64)
    print("append", sv.append(np.arange(1500, dtype=np.int64) + 100000, nb, nds), "shards", sv.count)
    settle(sv)
    assert sv.count == 3
    sv.set_option("device_merge", 1)
    print("batch over the grown set: hits", sv.query_batch(pb, po)[3])
    sv.close()
    # a three-rank group over three indexes
    cut = [0, 1000, 2000, 3000]
    shards = []
    for r in range(3):
        g = capi.GpuStringIndex()
        g.add_bulk(ids[cut[r]:cut[r + 1]], blob[int(ds[cut[r]]):int(ds[cut[r + 1]])], ds[cut[r]:cut[r + 1] + 1] - ds[cut[r]])
        g.build()
        g.proof_wait()
        shards.append(g)
    d_blob = torch.from_numpy(np.concatenate([pb, np.zeros(16, dtype=np.uint8)])).cuda()
    d_offs = torch.from_numpy(po.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    local = [g.query_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), len(po) - 1, len(pb)) for g in shards]
    comms = capi.ShardComm.group([0, 0, 0])
    print("merge rows", [int(m.nrows) for m in collective(lambda r: comms[r].merge(local[r]), 3)])
    print("merge_counts rows", [int(s.nrows_total) for s in collective(lambda r: comms[r].merge_counts(local[r]), 3)])
    for x in comms + shards:
        x.close()


if __name__ == "__main__":
    main()
