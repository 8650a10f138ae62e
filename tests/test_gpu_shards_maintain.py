"""Remove, append and cluster on a sharded string column (cdb_shards_remove / cdb_shards_append / cdb_shards_cluster,
capi.GpuShards.remove / .append / .cluster).  All shards live on device 0 (repeated device slots).  Two referees, neither of them
code under test: ONE GpuStringIndex freshly built over the same final column, and plain Python (a dict for cluster, set
arithmetic for removed / missing).  After every operation the sharded set must answer like the single index on every query
entry point, with the host merge and with the device merge, and again after save + load into a fresh set.

Two text kinds.  "ascii" takes the compaction / merge paths.  "high" holds bytes >= 0x80 under reference_compat = 1: the array is in
the reference's order and every change rebuilds it.  There the answers follow the reference's own search over that array, and once a
column outgrows the reference's bucket size (4096 suffixes, index.cpp:218) its radix nodes order bytes >= 0x80 as signed while the
search compares them as unsigned: the answers then depend on how many suffixes ONE array holds, so a sharded set and a single index
disagree even when both were just built (measured on an MI355X, 900 documents / 15 KB, fresh builds on both sides: b"aa" 478 rows
against 348).  Up to 4096 bytes an array is one sorted leaf and both sides answer exactly, so the "high" column and everything
appended to it stay below that size and are compared with the single index like the ASCII one; beyond it (the last test) every
shard is compared with a fresh index over that shard's own documents instead."""
import numpy as np
import pytest

from coffeedb_amd import capi

pytestmark = pytest.mark.gpu

KINDS = ["ascii", "high"]
ALPHABET = {"ascii": b"abc", "high": bytes([0x61, 0xC3, 0xA9, 0x62])}   # "high": bytes >= 0x80 (reference order under reference_compat)
ABSENT = b"\x01"                                                        # a byte no corpus holds


# ---- helpers -----------------------------------------------------------------------------------------------------------
def pack(docs):
    blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    return blob, ds


SIZES = {"ascii": (900, 2), "high": (160, 8)}   # documents, and every k-th of them is a long one ("high": the column stays below 4096 bytes)
LEAF = 4096


def corpus(kind, n, seed, long_every=None):
    """n documents of 0..64 bytes over a 3-4 letter alphabet, every k-th one long and the others at most 4 bytes: equal documents,
    equal suffixes and empty documents are common, and the same strings turn up in every part of the column"""
    rng = np.random.default_rng(seed)
    al = np.frombuffer(ALPHABET[kind], dtype=np.uint8)
    k = long_every or SIZES[kind][1]
    docs = []
    for d in range(n):
        ln = int(rng.integers(0, 5)) if d % k else int(rng.integers(0, 65))
        docs.append(bytes(al[rng.integers(0, len(al), size=ln)]))
    twin = bytes(al[[0, 1, 0, 2, 1, 0, 0]])
    for d in (3, n // 2, n - 4):      # equal documents planted in the first, a middle and the last part
        docs[d] = twin
    for d in (5, n // 2 + 1, n - 2):  # ... and the empty document
        docs[d] = b""
    return docs


def options(kind):
    return {"reference_compat": 1} if kind == "high" else {}


def single(ids, docs, kind):
    g = capi.GpuStringIndex(device=0)
    for k, v in options(kind).items():
        g.set_option(k, v)
    blob, ds = pack(docs)
    g.add_bulk(np.asarray(ids, dtype=np.int64), blob, ds)
    g.build()
    return g


def sharded(ids, docs, kind, slots=3, spread=True, **opts):
    sh = capi.GpuShards([0] * slots)
    if spread:
        sh.set_option("use_all_devices", 1)
    for k, v in {**options(kind), **opts}.items():
        sh.set_option(k, v)
    if len(ids):
        blob, ds = pack(docs)
        sh.add_bulk(np.asarray(ids, dtype=np.int64), blob, ds)
        sh.build()
    return sh


def keywords(kind):
    a = ALPHABET[kind]
    return [a[0:1], a[1:2], a[2:3], a[0:2], a[1:3], a[0:1] * 2, a[0:1] + a[2:3], a[0:3], a[1:2] + a[0:1] + a[1:2],
            bytes([a[0], a[1], a[0], a[2]]), bytes([a[2], a[2], a[1], a[0], a[0]]), ABSENT]


def cluster_by_dict(ids, docs, rows):
    """database.cpp:442-460 over the rows whose id the column holds"""
    doc_of = {int(i): d for i, d in zip(ids, docs)}
    groups, missing = {}, 0
    for r in rows:
        if int(r) not in doc_of:
            missing += 1
            continue
        c, rep = groups.get(doc_of[int(r)], (0, None))
        groups[doc_of[int(r)]] = (c + 1, int(r) if rep is None else min(rep, int(r)))
    values = sorted(groups)          # bytes compare as std::string does: unsigned, a proper prefix first
    return values, [groups[v][0] for v in values], [groups[v][1] for v in values], missing


def check_cluster(sh, one, ids, docs, rows):
    rows = np.asarray(rows, dtype=np.int64)
    values, counts, reps, missing = cluster_by_dict(ids, docs, rows)
    for with_values in (True, False):
        gv, gc, gr, gm = sh.cluster(rows, with_values=with_values)
        assert sum(int(c) for c in gc) + gm == len(rows)
        assert gv == (values if with_values else None)
        assert list(gc) == counts and list(gr) == reps and gm == missing
        ov, oc, orr, om = one.cluster(rows, with_values=with_values)
        assert gv == ov and list(gc) == list(oc) and list(gr) == list(orr) and gm == om


def cluster_rows(ids):
    """every id, some twice, and ids nobody holds"""
    ids = [int(i) for i in ids]
    top = max(ids) if ids else 0
    return ids + ids[::5] + [top + 7, top + 7, -5]


def same_answers(sh, one, kind):
    kws = keywords(kind)
    for kw in kws:
        assert sh.query(kw) == one.query(kw), kw
    pb, po = pack(kws)
    want = one.query_batch(pb, po)
    for merge in (0, 1):
        sh.set_option("device_merge", merge)
        got = sh.query_batch(pb, po)
        assert got[3] == want[3] and all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])), f"device_merge={merge}"
        go, wo = sh.query_batch_offsets(pb, po), one.query_batch_offsets(pb, po)
        assert all(np.array_equal(a, b) for a, b in zip(go, wo)), f"device_merge={merge}"
    sh.set_option("device_merge", 0)
    assert sh.query_or(kws[:6]) == one.query_or(kws[:6])
    assert sh.query_or(kws, ranked=True, lo=2, limit=25) == one.query_ranked(kws, lo=2, limit=25)
    assert sh.query_or(kws[:4], ranked=True) == one.query_ranked(kws[:4])
    assert sh.query_spans(kws[3:8]) == one.query_spans(kws[3:8])


def check_all(sh, ids, docs, kind, tmp_path, tag=""):
    """the sharded set against ONE fresh index over (ids, docs), then once more after save + load into a fresh set"""
    assert kind != "high" or total_bytes(docs) <= LEAF   # (one sorted leaf on both sides: see the module text)
    one = single(ids, docs, kind)
    nshards = sh.count
    assert sh.first_doc(0) == 0 and sh.first_doc(nshards) == len(ids)
    page = [int(i) for i in ids[::max(1, len(ids) // 40)]] + [-9]
    for s in (sh, None):
        if s is None:               # save, then load into a fresh set
            if nshards < 1:
                break
            path = str(tmp_path / f"saved{tag}")
            sh.save(path)
            s = capi.GpuShards([0] * nshards)
            for k, v in options(kind).items():
                s.set_option(k, v)
            s.load(path)
            assert s.count == nshards and [s.first_doc(i) for i in range(nshards + 1)] == [sh.first_doc(i) for i in range(nshards + 1)]
        same_answers(s, one, kind)
        a = s.render_rows(page, keywords(kind)[:5], left=b"<", right=b">")
        b = one.render_rows(page, keywords(kind)[:5], left=b"<", right=b">")
        assert list(a[0]) == list(b[0]) and a[1:] == b[1:]
        check_cluster(s, one, ids, docs, cluster_rows(ids))
        check_cluster(s, one, ids, docs, [])
        if s is not sh:
            s.close()
    one.close()


def bounds_of(sh):
    return [sh.first_doc(i) for i in range(sh.count + 1)]


def shard_stats(sh, names=("removes", "remove_compactions", "remove_rebuilds", "appends", "append_merges", "append_rebuilds")):
    return [[sh.shard(i).stat(n) for n in names] for i in range(sh.count)]


def survivors(ids, docs, gone):
    gone = set(int(x) for x in gone)
    keep = [k for k, i in enumerate(ids) if int(i) not in gone]
    return [ids[k] for k in keep], [docs[k] for k in keep]


def total_bytes(docs):
    return sum(len(d) for d in docs)


@pytest.fixture(scope="module", params=KINDS)
def column(request):
    kind = request.param
    n = SIZES[kind][0]
    return kind, [1000 + 3 * d for d in range(n)], corpus(kind, n, seed=11 if kind == "ascii" else 12)


# ---- remove ------------------------------------------------------------------------------------------------------------
REMOVALS = ["one_shard", "every_shard", "middle_all", "first_all", "last_all", "everything", "mixed", "nothing"]


@pytest.mark.parametrize("which", REMOVALS)
def test_remove(column, which, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh = sharded(ids, docs, kind)
    b = bounds_of(sh)
    assert sh.count == 3 and b[0] == 0 and b[3] == N
    part = [ids[b[i]:b[i + 1]] for i in range(3)]
    gone = {
        "one_shard": part[1][2::3],
        "every_shard": part[0][::4] + part[1][1::2] + part[2][-7:],
        "middle_all": part[1],
        "first_all": part[0],
        "last_all": part[2],
        "everything": list(reversed(ids)),
        "mixed": [part[0][1], 5, part[2][3], part[0][1], 999999, 5, part[1][0], part[2][3], part[2][3]],   # held, twice, and nobody's
        "nothing": [],
    }[which]
    held = set(ids)
    want_removed = len(held & set(gone))
    want_missing = sum(1 for x in gone if x not in held)
    removed, missing = sh.remove(gone)
    assert (removed, missing) == (want_removed, want_missing)
    kids, kdocs = survivors(ids, docs, gone)
    # an emptied shard stays in place: the count holds, the bounds follow the surviving documents of every shard
    assert sh.count == 3
    left = [len(set(p) - set(gone)) for p in part]
    assert bounds_of(sh) == [0, left[0], left[0] + left[1], len(kids)]
    for i in range(3):
        touched = bool(set(part[i]) & set(gone))
        st = sh.shard(i)
        assert st.stat("removes") == (1 if touched else 0)
        assert st.stat("remove_compactions") == (1 if touched and kind == "ascii" else 0)
        assert st.stat("remove_rebuilds") == (1 if touched and kind == "high" else 0)
    check_all(sh, kids, kdocs, kind, tmp_path)
    sh.close()


def test_remove_from_a_set_never_built(column):
    kind, ids, docs = column
    sh = sharded([], [], kind)
    assert sh.count == 0
    assert sh.remove([1, 2, 2, 7]) == (0, 4)
    assert sh.remove([]) == (0, 0)
    assert sh.count == 0 and sh.query(b"a") == []
    values, counts, reps, missing = sh.cluster([1, 2, 2])
    assert values == [] and len(counts) == 0 and len(reps) == 0 and missing == 3
    values, counts, reps, missing = sh.cluster([])
    assert values == [] and len(counts) == 0 and missing == 0
    sh.close()


def test_remove_is_refused_after_add(column, tmp_path):
    kind, ids, docs = column
    sh = sharded(ids, docs, kind)
    before_bounds, before_stats = bounds_of(sh), shard_stats(sh)
    sh.add(77, b"abc")
    with pytest.raises(RuntimeError, match="remove: documents were added since the last build"):
        sh.remove(ids[:10])
    with pytest.raises(RuntimeError, match="append: documents were added since the last build"):
        sh.append([78], *pack([b"ab"]))
    assert bounds_of(sh) == before_bounds and shard_stats(sh) == before_stats
    check_all(sh, ids, docs, kind, tmp_path)           # every answer unchanged: the staged document is not served
    sh.build()                                           # ... and still staged: the build brings it in
    check_all(sh, ids + [77], docs + [b"abc"], kind, tmp_path, tag="_built")
    sh.close()


# ---- append ------------------------------------------------------------------------------------------------------------
def fresh_docs(kind, n, seed, first_id):
    return [first_id + 2 * d for d in range(n)], corpus(kind, max(n, 12), seed)[:n]


def two_of_four(ids, docs, kind, slots=4):
    """two shards in use, idle slots behind them: max_shard_bytes = 0.6 of the column"""
    limit = total_bytes(docs) * 6 // 10
    sh = sharded(ids, docs, kind, slots=slots, spread=False, max_shard_bytes=limit)
    assert sh.count == 2
    return sh, limit


def test_append_into_the_last_shard_when_it_fits(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh, limit = two_of_four(ids, docs, kind)
    nids, ndocs = fresh_docs(kind, N // 22, 21, 50000)  # ~ 4 % of the column: the last shard stays within the limit
    assert total_bytes(docs[sh.first_doc(1):]) + total_bytes(ndocs) <= limit
    assert sh.append(nids, *pack(ndocs)) == len(nids)
    assert sh.count == 2 and bounds_of(sh)[2] == N + len(nids)
    assert [sh.shard(i).stat("appends") for i in range(2)] == [0, 1]
    assert sh.shard(1).stat("append_merges" if kind == "ascii" else "append_rebuilds") == 1
    check_all(sh, ids + nids, docs + ndocs, kind, tmp_path)
    sh.close()


def test_append_opens_one_new_shard(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh, limit = two_of_four(ids, docs, kind)
    old_bounds = bounds_of(sh)
    nids, ndocs = fresh_docs(kind, N // 3, 22, 50000)
    assert total_bytes(docs[sh.first_doc(1):]) + total_bytes(ndocs) > limit >= total_bytes(ndocs)
    assert sh.append(nids, *pack(ndocs)) == len(nids)
    assert sh.count == 3 and bounds_of(sh) == old_bounds + [N + len(nids)]      # the old shards stay as they are
    assert [sh.shard(i).stat("appends") for i in range(2)] == [0, 0]
    check_all(sh, ids + nids, docs + ndocs, kind, tmp_path)                     # (device merge with the new shard count included)
    sh.close()


def test_append_needs_more_pieces_than_idle_slots(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh, limit = two_of_four(ids, docs, kind)
    nids, ndocs = fresh_docs(kind, 2 * N + N // 4, 23, 50000)
    assert total_bytes(ndocs) > 3 * limit                # four pieces would be needed, two slots are idle
    assert sh.append(nids, *pack(ndocs)) == len(nids)
    b = bounds_of(sh)
    assert sh.count == 4 and b[4] == N + len(nids)
    assert total_bytes(ndocs[:b[3] - N]) <= limit < total_bytes(ndocs[:b[3] - N + 1])   # the first piece is full, the last takes the rest
    check_all(sh, ids + nids, docs + ndocs, kind, tmp_path)
    sh.close()


def test_append_with_no_idle_slot_left(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh, limit = two_of_four(ids, docs, kind, slots=2)
    nids, ndocs = fresh_docs(kind, N // 3, 24, 50000)
    assert total_bytes(docs[sh.first_doc(1):]) + total_bytes(ndocs) > limit
    assert sh.append(nids, *pack(ndocs)) == len(nids)
    assert sh.count == 2 and bounds_of(sh)[2] == N + len(nids)
    assert [sh.shard(i).stat("appends") for i in range(2)] == [0, 1]
    check_all(sh, ids + nids, docs + ndocs, kind, tmp_path)
    sh.close()


def test_append_to_a_set_never_built(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh = sharded([], [], kind, slots=3, spread=False, max_shard_bytes=total_bytes(docs) * 6 // 10)
    assert sh.append([], *pack([])) == 0 and sh.count == 0
    assert sh.append(ids, *pack(docs)) == N
    assert sh.count == 2                                 # cdb_shards_build_views' own cut
    check_all(sh, ids, docs, kind, tmp_path)
    sh.close()


def test_append_nothing_and_empty_documents(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh = sharded(ids, docs, kind)
    before_bounds, before_stats = bounds_of(sh), shard_stats(sh)
    assert sh.append([], *pack([])) == 0
    assert bounds_of(sh) == before_bounds and shard_stats(sh) == before_stats
    assert sh.append([70001, 70002, 70003], *pack([b"", b"", b""])) == 3       # empty documents only
    nids, ndocs = [70010, 70011, 70012, 70013], [b"", ALPHABET[kind][:2], b"", ALPHABET[kind]]
    assert sh.append(nids, *pack(ndocs)) == 4
    assert sh.count == 3 and bounds_of(sh)[3] == N + 7
    check_all(sh, ids + [70001, 70002, 70003] + nids, docs + [b"", b"", b""] + ndocs, kind, tmp_path)
    sh.close()


def test_remove_append_remove_add_build(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh = sharded(ids, docs, kind)
    gone = ids[1::3]
    assert sh.remove(gone) == (len(gone), 0)
    cids, cdocs = survivors(ids, docs, gone)
    nids, ndocs = fresh_docs(kind, N // 8, 25, 50000)
    assert sh.append(nids, *pack(ndocs)) == N // 8
    cids, cdocs = cids + nids, cdocs + ndocs
    check_all(sh, cids, cdocs, kind, tmp_path, tag="_1")
    gone = cids[::7] + [4]
    assert sh.remove(gone) == (len(gone) - 1, 1)
    cids, cdocs = survivors(cids, cdocs, gone)
    check_all(sh, cids, cdocs, kind, tmp_path, tag="_2")
    sh.add(90001, ALPHABET[kind] * 3)                    # the staging copy was dropped: the survivors are fetched back from the shards
    sh.build()
    cids, cdocs = cids + [90001], cdocs + [ALPHABET[kind] * 3]
    check_all(sh, cids, cdocs, kind, tmp_path, tag="_3")
    assert sh.remove([90001]) == (1, 0)                  # ... and a built set takes the next change
    check_all(sh, cids[:-1], cdocs[:-1], kind, tmp_path, tag="_4")
    sh.close()


# ---- cluster -----------------------------------------------------------------------------------------------------------
def test_cluster_fuses_groups_across_shards(column):
    kind, ids, docs = column
    N = len(ids)
    sh = sharded(ids, docs, kind)
    one = single(ids, docs, kind)
    b = bounds_of(sh)
    twins = [d for d in range(N) if docs[d] == docs[3]]
    empties = [d for d in range(N) if docs[d] == b""]
    shard_of = lambda d: max(i for i in range(3) if b[i] <= d)   # noqa: E731
    assert len({shard_of(d) for d in twins}) == 3 and len({shard_of(d) for d in empties}) >= 2   # planted in different shards
    rows = [ids[d] for d in twins + empties]
    values, counts, reps, missing = sh.cluster(rows)
    assert values == [b"", docs[3]] and list(counts) == [len(empties), len(twins)] and missing == 0
    assert list(reps) == [ids[min(empties)], ids[min(twins)]]
    check_cluster(sh, one, ids, docs, rows)
    check_cluster(sh, one, ids, docs, cluster_rows(ids))            # repeated ids, ids nobody holds
    check_cluster(sh, one, ids, docs, [-1, -2, 999999])             # nobody's only
    check_cluster(sh, one, ids, docs, [])                           # nrows = 0
    one.close()
    sh.close()


# ---- all or nothing ----------------------------------------------------------------------------------------------------
def refused(sh, ids, docs, kind, tmp_path, call, match, tag):
    """after a refused call: every answer, the per-shard stats and the bounds are what they were"""
    before_bounds, before_stats, before_count = bounds_of(sh), shard_stats(sh), sh.count
    with pytest.raises(RuntimeError, match=match):
        call()
    assert sh.count == before_count and bounds_of(sh) == before_bounds and shard_stats(sh) == before_stats
    check_all(sh, ids, docs, kind, tmp_path, tag=tag)


def test_refused_calls_change_nothing(column, tmp_path):
    kind, ids, docs = column
    N = len(ids)
    sh, limit = two_of_four(ids, docs, kind)
    nids, ndocs = fresh_docs(kind, N // 3, 26, 50000)
    blob, ds = pack(ndocs)
    bad = ds.copy()
    bad[5] = bad[7] + 1                                  # doc_start runs backwards in the middle of the batch
    refused(sh, ids, docs, kind, tmp_path, lambda: sh.append(nids, blob, bad), "doc_start must be non-decreasing", "_a")
    # the batch would open a new shard, whose build fails (test hook, thrown on the host; an option set on the SET, so it reached
    # the new shard's fresh handle): that handle is dropped
    sh.set_option("debug_fail_build", 1)
    refused(sh, ids, docs, kind, tmp_path, lambda: sh.append(nids, blob, ds), "build failure requested", "_b")
    if kind == "ascii":
        # a small batch joins the last shard through the merge, whose inner build fails: the prepared column is dropped
        refused(sh, ids, docs, kind, tmp_path, lambda: sh.append(nids[:N // 30], *pack(ndocs[:N // 30])), "build failure requested", "_c")
    sh.set_option("debug_fail_build", 0)
    assert sh.append(nids, blob, ds) == len(nids) and sh.count == 3
    check_all(sh, ids + nids, docs + ndocs, kind, tmp_path, tag="_d")
    sh.close()


def test_failed_build_behind_the_commit_leaves_that_shard_never_built(tmp_path):
    # the reference-order path builds the array over the new text AFTER the shard's commit; the header says what a caller finds
    # when that build fails on one shard: its error, that shard "never built" (its documents are gone), every other shard
    # committed, the count unchanged and the bounds describing exactly what is still served
    kind = "high"
    N = SIZES[kind][0]
    ids, docs = [1000 + 3 * d for d in range(N)], corpus(kind, N, seed=12)
    sh = sharded(ids, docs, kind)
    b = bounds_of(sh)
    part = [ids[b[i]:b[i + 1]] for i in range(3)]
    gone = part[0][::2] + part[1][::2] + part[2][::2]
    sh.shard(1).set_option("debug_fail_build", 1)        # (test hook, thrown on the host)
    with pytest.raises(RuntimeError, match="build failure requested"):
        sh.remove(gone)
    sh.shard(1).set_option("debug_fail_build", 0)
    kids, kdocs = survivors(ids, docs, gone + part[1])
    assert sh.count == 3 and bounds_of(sh) == [0, len(part[0][1::2]), len(part[0][1::2]), len(kids)]
    one = single(kids, kdocs, kind)
    same_answers(sh, one, kind)
    check_cluster(sh, one, kids, kdocs, cluster_rows(ids))
    one.close()
    sh.close()


def test_reference_order_beyond_one_leaf_every_shard_equals_a_fresh_build():
    # 900 documents (15 KB) with bytes >= 0x80 under reference_compat = 1: the arrays have radix nodes, where only a shard and a fresh
    # index over THAT SHARD's documents can be compared (see the module text).  After a removal from every shard and an append into the
    # last one, every shard cannot be told from such an index: layout, suffix array, queries
    kind = "high"
    n = 900
    ids, docs = [1000 + 3 * d for d in range(n)], corpus(kind, n, seed=13, long_every=2)
    sh = sharded(ids, docs, kind)
    b = bounds_of(sh)
    assert min(total_bytes(docs[b[i]:b[i + 1]]) for i in range(3)) > LEAF
    gone = ids[::3]
    assert sh.remove(gone) == (len(gone), 0)
    cids, cdocs = survivors(ids, docs, gone)
    nids, ndocs = [50000 + d for d in range(100)], corpus(kind, 100, seed=14, long_every=2)
    assert sh.append(nids, *pack(ndocs)) == 100
    cids, cdocs = cids + nids, cdocs + ndocs
    b = bounds_of(sh)
    assert sh.count == 3 and b[3] == len(cids)
    assert [sh.shard(i).stat("remove_rebuilds") for i in range(3)] == [1, 1, 1] and sh.shard(2).stat("append_rebuilds") == 1
    pb, po = pack(keywords(kind))
    for i in range(3):
        g, f = sh.shard(i), single(cids[b[i]:b[i + 1]], cdocs[b[i]:b[i + 1]], kind)
        assert (g.size, g.bits, g.mask, g.sa_width) == (f.size, f.bits, f.mask, f.sa_width)
        assert np.array_equal(g.sa(), f.sa())
        got, want = g.query_batch(pb, po), f.query_batch(pb, po)
        assert got[3] == want[3] and all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3]))
        assert g.verify_reference()["violations"] == 0
        f.close()
    check_cluster(sh, single(cids, cdocs, kind), cids, cdocs, cluster_rows(cids))   # (cluster never searches: exact at any size)
    sh.close()
