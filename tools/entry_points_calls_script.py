"""One fixed piece of work through the query-side entry points for a call-count comparison of two libraries
(tools/build_calls_compare.py is the comparer; tools/shards_calls_script.py is its counterpart for the sharded index): over eight
short documents, one int64 column of the same rows and two co-resident shards on one device, every entry point whose host half
goes through keyword_list.h / host_io.h is called once with an answer that has rows — and cdb_query_or, cdb_query_ranked,
cdb_query_and and cdb_query_and_columns once more with an answer that has none (EMPTY_ROW_CALLS of them: the calls whose download
synchronises an idle stream where it used to return without).  Run it under `rocprofv3 --kernel-trace --hip-trace --stats` once
per library (CDB_LIB_PATH); every order proof is awaited, so that every run makes the same calls."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coffeedb_amd import capi  # noqa: E402

DOCS = [b"3010103", b"301022", b"01011010", b"abcabcabc", b"aaaaaa", b"banana 010", b"coffee 0101 abc", b"tea"]
KW1, KW2, ABSENT = [b"010", b"abc"], [b"0", b"a"], [b"zzz"]
EMPTY_ROW_CALLS = 4


def main():
    ids = np.arange(len(DOCS), dtype=np.int64) + 100
    blob = np.frombuffer(b"".join(DOCS), dtype=np.uint8)
    ds = np.array(np.cumsum([0] + [len(d) for d in DOCS]), dtype=np.uint64)
    one = capi.GpuStringIndex(device=0)
    one.add_bulk(ids, blob, ds)
    one.build()
    one.proof_wait()
    sh = capi.GpuShards([0, 0])
    sh.set_option("use_all_devices", 1)
    sh.add_bulk(ids, blob, ds)
    sh.build()
    for i in range(sh.count):
        sh.shard(i).proof_wait()
    col = capi.GpuColumn("int64", device=0)
    col.add_bulk(ids, np.arange(len(DOCS)) + 1)
    col.build()
    pb = np.frombuffer(b"".join(KW1), dtype=np.uint8)
    po = np.array([0, 3, 6], dtype=np.uint64)
    host_rows = [(100, 0), (101, 0), (102, 0), (105, 0), (106, 0), (107, 0)]

    print("batch", one.query_batch(pb, po)[3], "with offsets", len(one.query_batch_offsets(pb, po)[4]))
    one.set_option("coalesce_queries", 0)
    print("query", one.query(b"010"))
    print("or", one.query_or(KW1), "ranked", one.query_ranked(KW1, limit=3), "spans", len(one.query_spans(KW1)))
    keys = [(one, KW1), (one, KW2), (None, host_rows)]
    print("and", capi.query_and(keys), "ranked", capi.query_and(keys, ranked=True, limit=3))
    print("and + column", capi.query_and(keys + [(col, ["[2,6]"])]))
    with capi.filter_rows(keys + [(col, ["[2,6]"])]) as rs:
        print("filter", len(rs), rs.rows()[0], rs.page(0, 2)[0], rs.cluster(one)[0], rs.cluster(col)[0])
        print("select", rs.select(0, 2, [(one, KW1), (sh, KW1), col], left=b"<b>", right=b"</b>")[0])
    with capi.rowset_all([one, col]) as rs:
        print("all", len(rs))
    print("render", one.render_rows([107, 100, 999], KW1, left=b"<b>", right=b"</b>")[3], "cluster", one.cluster(ids)[0][:2], col.cluster(ids)[0][:2])
    print("column", col.query("[2,6]"), col.query_any(["[1,2]", "[7,9]"]), col.values(ids[:3]))
    for dm in (0, 1):
        sh.set_option("device_merge", dm)
        print("shards batch device_merge", dm, "hits", sh.query_batch(pb, po)[3])
    sh.set_option("device_merge", 0)
    print("shards query", sh.query(b"010"), "or", sh.query_or(KW1), "render", sh.render_rows([107, 100, 999], KW1)[3])
    print("shards and", capi.query_and([(sh, KW1), (sh, KW2), (None, host_rows)]))
    # the answers without rows
    print("empty", one.query_or(ABSENT), one.query_ranked(ABSENT), capi.query_and([(one, ABSENT), (None, host_rows)]),
          capi.query_and([(one, ABSENT), (col, ["[2,6]"])]))
    for h in (col, sh, one):
        h.close()


if __name__ == "__main__":
    main()
