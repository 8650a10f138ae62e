"""`cluster` on the GPU (cdb_column_cluster / cdb_cluster, capi.GpuColumn.cluster / GpuStringIndex.cluster) against the
reference's algorithm (database.cpp:442-460) restated here: a collections.Counter over the values the given ids hold, printed
with str(int) / "%f" % v / "0", "1" for the numeric kinds and ordered by the encoded bytes; for the device's own groups the
distinct values ascending with their counts, the smallest id of each group and the number of rows the column does not hold.
Every comparison is exact equality."""
import collections
import os
import struct
import threading

import numpy as np
import pytest

from coffeedb_amd import capi, workloads as W

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
PATHS = {"auto": 0, "sparse": 1, "dense": 2}


# ---- the model ---------------------------------------------------------------------------------------------------------
def _fold(kind, v):
    """The column's one divergence from the reference (coffeedb_gpu.h): a double column folds -0.0 onto +0.0 when it is built."""
    return 0.0 if kind == 2 and v == 0 else v


def _printed(kind, v):
    if kind == 1:
        return str(int(v))
    if kind == 2:
        return "%f" % v
    return "1" if v else "0"


def model_groups(kind, store, ids):
    """(values ascending, counts, smallest id per group, missing) — what the device returns."""
    cnt, rep, missing = collections.Counter(), {}, 0
    for i in ids:
        i = int(i)
        if i not in store:
            missing += 1
            continue
        v = _fold(kind, store[i])
        cnt[v] += 1
        rep[v] = min(rep.get(v, i), i)
    vals = sorted(cnt)
    return vals, [cnt[v] for v in vals], [rep[v] for v in vals], missing


def model_printed(kind, store, ids):
    """database.cpp:442-460: std::map<std::string, int64_t> over the printed values (rows the store lacks skipped)."""
    cnt = collections.Counter(_printed(kind, _fold(kind, store[int(i)])) for i in ids if int(i) in store)
    return sorted(cnt.items(), key=lambda kv: kv[0].encode())


def printed_of_device(kind, values, counts):
    """shim/cluster.h: cluster_rows over the device's groups."""
    cnt = collections.Counter()
    for v, c in zip(values.tolist(), counts.tolist()):
        cnt[_printed(kind, v)] += c
    return sorted(cnt.items(), key=lambda kv: kv[0].encode())


def check_column(col, kind, store, ids):
    values, counts, reps, missing = col.cluster(ids)
    mv, mc, mr, mm = model_groups(kind, store, ids)
    assert missing == mm
    assert counts.tolist() == mc
    assert reps.tolist() == mr
    if kind == 2:   # bit for bit: +0.0 stands for both zeros
        assert [struct.pack("<d", v) for v in values.tolist()] == [struct.pack("<d", v) for v in mv]
    else:
        assert values.tolist() == ([bool(v) for v in mv] if kind == 0 else mv)
    assert int(counts.sum()) + missing == len(ids)
    assert printed_of_device(kind, values, counts) == model_printed(kind, store, ids)


def column_data(kind, n, seed):
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(-n // 2, n - n // 2, dtype=np.int64) * 977 + 13)  # negative and non-ascending
    if kind == 1:
        pool = np.array([I64_MIN, I64_MIN + 1, -10, -1, 0, 1, 9, 10, 999, 1234, I64_MAX - 1, I64_MAX], dtype=np.int64)
        vals = pool[rng.integers(0, len(pool), n)]
        vals[: n // 8] = rng.integers(-50, 50, n // 8)
    elif kind == 2:
        pool = np.array([-np.inf, -2.5, -1e-7, -0.0, 0.0, 1e-7, 2e-7, 4.9e-7, 1.5, 1234567.125, 1e300, np.inf], dtype=np.float64)
        vals = pool[rng.integers(0, len(pool), n)]
        vals[: n // 8] = np.round(rng.normal(0, 3, n // 8), 1)
    else:
        vals = rng.integers(0, 2, n).astype(np.uint8)
    return ids, vals


def make_column(kind, ids, vals):
    col = capi.GpuColumn(kind, device=0)
    col.add_bulk(ids, vals)
    col.build()
    return col


def store_of(kind, ids, vals):
    conv = {0: bool, 1: int, 2: float}[kind]
    return {int(i): conv(v) for i, v in zip(ids.tolist(), vals.tolist())}


# ---- columns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("kind", [1, 2, 0])
def test_column_cluster_against_model(kind, path):
    n = 3000
    ids, vals = column_data(kind, n, seed=100 + kind)
    store = store_of(kind, ids, vals)
    col = make_column(kind, ids, vals)
    col.set_option("debug_cluster_path", PATHS[path])
    rng = np.random.default_rng(7)
    check_column(col, kind, store, ids)                                              # (a) every row
    check_column(col, kind, store, ids[rng.permutation(n)[:37]])                     #     a few rows
    mixed = np.concatenate([ids[:500], ids[:200], ids[100:103], np.array([5, 6, I64_MIN, I64_MAX, 10 ** 15], dtype=np.int64),
                            ids[2000:]])
    check_column(col, kind, store, mixed[rng.permutation(len(mixed))])               # (c) repeated ids and ids never seen
    check_column(col, kind, store, np.array([5, 6, 7], dtype=np.int64))              #     nothing but strangers
    check_column(col, kind, store, np.empty(0, dtype=np.int64))                      # (d) the empty list
    if kind != 0 and path != "auto":
        assert col.stat("sparse_clusters" if path == "sparse" else "dense_clusters") >= 4
        assert col.stat("dense_clusters" if path == "sparse" else "sparse_clusters") == 0
    col.close()


@pytest.mark.parametrize("kind", [1, 2, 0])
def test_unbuilt_column_has_no_groups(kind):
    col = capi.GpuColumn(kind, device=0)
    ids = np.array([3, 1, 2, 3], dtype=np.int64)
    values, counts, reps, missing = col.cluster(ids)                                 # (e) never built
    assert (len(values), len(counts), len(reps), missing) == (0, 0, 0, 4)
    col.add_bulk(ids[:3], np.array([1, 0, 1]))
    values, counts, reps, missing = col.cluster(ids)                                 # staged rows are not visible yet
    assert (len(values), missing) == (0, 4)
    assert col.cluster(np.empty(0, dtype=np.int64))[3] == 0
    col.close()


def test_negative_zero_folds_onto_positive_zero():
    # the documented divergence: the reference would print "-0.000000" and "0.000000" as two entries
    col = make_column(2, np.array([10, 11, 12, 13], dtype=np.int64), np.array([-0.0, 0.0, -0.0, 1.0]))
    for path in PATHS.values():
        col.set_option("debug_cluster_path", path)
        values, counts, reps, missing = col.cluster(np.array([13, 12, 11, 10], dtype=np.int64))
        assert [struct.pack("<d", v) for v in values.tolist()] == [struct.pack("<d", 0.0), struct.pack("<d", 1.0)]
        assert counts.tolist() == [3, 1] and reps.tolist() == [10, 13] and missing == 0
    col.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_cluster_rows_of_a_device_filter(path):
    # (b) the rows cdb_query_and_columns returns for a string key AND a range, clustered by a third field
    nd = 4000
    blob, ds = W.ascii_corpus(nd, 48, seed=21)
    ids = np.arange(nd, dtype=np.int64) * 3 + 1000
    rng = np.random.default_rng(3)
    age = rng.integers(0, 90, nd).astype(np.int64)
    score = np.round(rng.normal(0, 2, nd), 1)
    g = capi.GpuStringIndex(device=0)
    g.add_bulk(ids, blob, ds)
    g.build()
    c_age, c_score = make_column(1, ids, age), make_column(2, ids, score)
    kw = bytes(blob[int(ds[5]):int(ds[5]) + 1])   # one byte: a few hundred documents hold it
    rows = capi.query_and([(g, [kw]), (c_age, ["[20,60)"])])
    rid = np.array([r[0] for r in rows], dtype=np.int64)
    assert 10 < len(rid) < nd
    for col, kind, vals in ((c_age, 1, age), (c_score, 2, score)):
        col.set_option("debug_cluster_path", PATHS[path])
        check_column(col, kind, store_of(kind, ids, vals), rid)
    for x in (g, c_age, c_score):
        x.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_cluster_follows_a_rebuilt_column(path):
    ids, vals = column_data(1, 2000, seed=5)
    col = make_column(1, ids[:1200], vals[:1200])
    col.set_option("debug_cluster_path", PATHS[path])
    check_column(col, 1, store_of(1, ids[:1200], vals[:1200]), ids)                  # 800 rows still unknown
    col.add_bulk(ids[1200:], vals[1200:])
    check_column(col, 1, store_of(1, ids[:1200], vals[:1200]), ids)                  # ... and invisible before the build
    col.build()
    check_column(col, 1, store_of(1, ids, vals), ids)
    col.close()


def test_midsize_column_multi_block_paths():
    n = 10 ** 7
    rng = np.random.default_rng(11)
    ids = np.arange(n, dtype=np.int64) * 5 + 17
    vals = (rng.integers(0, 1000, n).astype(np.int64) - 500) * 1000003
    col = make_column(1, ids, vals)
    for frac in (0.01, 0.9):
        sel = np.flatnonzero(rng.random(n) < frac)
        rows = ids[sel][rng.permutation(len(sel))]
        uv, first, uc = np.unique(vals[sel], return_index=True, return_counts=True)  # (ids ascend with the row index)
        for path in PATHS.values():
            col.set_option("debug_cluster_path", path)
            values, counts, reps, missing = col.cluster(rows)
            assert missing == 0
            assert np.array_equal(values, uv) and np.array_equal(counts, uc) and np.array_equal(reps, ids[sel][first])
    assert col.stat("sparse_clusters") >= 2 and col.stat("dense_clusters") >= 2
    col.close()


# ---- string indexes ----------------------------------------------------------------------------------------------------
def string_model(store, ids):
    cnt, rep, missing = collections.Counter(), {}, 0
    for i in ids:
        i = int(i)
        if i not in store:
            missing += 1
            continue
        d = store[i]
        cnt[d] += 1
        rep[d] = min(rep.get(d, i), i)
    docs = sorted(cnt)  # bytes compare as std::string does: unsigned, a proper prefix first, b"" first of all
    return docs, [cnt[d] for d in docs], [rep[d] for d in docs], missing


def check_strings(g, store, ids):
    values, counts, reps, missing = g.cluster(ids)
    md, mc, mr, mm = string_model(store, ids)
    assert missing == mm
    assert values == md
    assert counts.tolist() == mc and reps.tolist() == mr
    assert int(counts.sum()) + missing == len(ids)
    v2, c2, r2, m2 = g.cluster(ids, with_values=False)
    assert v2 is None and c2.tolist() == mc and r2.tolist() == mr and m2 == mm


def build_strings(docs, ids, **opts):
    g = capi.GpuStringIndex(device=0)
    for k, v in opts.items():
        g.set_option(k, v)
    lens = np.array([len(d) for d in docs], dtype=np.uint64)
    ds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
    g.add_bulk(ids, blob if len(blob) else np.zeros(1, dtype=np.uint8), ds)
    g.build()
    return g


def pooled_docs(nd, seed, lo=0x61, hi=0x66, long_doc=0):
    """nd documents drawn from a pool so that many repeat: empty ones, proper prefixes of others, documents equal to a
    suffix of another, and (long_doc > 0) one duplicated pair of that length."""
    rng = np.random.default_rng(seed)
    pool = [b"", b"ab", b"abc", b"abd", b"zab", b"b", b"a", b"abcabc", b"zabzab"]
    pool += [bytes(W.random_bytes(int(rng.integers(1, 6)), seed * 1000 + k, lo, hi)) for k in range(60)]
    docs = [pool[int(k)] for k in rng.integers(0, len(pool), nd)]
    if long_doc:
        big = bytes(W.random_bytes(long_doc, seed + 77, lo, hi))
        docs[nd // 3] = big
        docs[2 * nd // 3] = big
        docs[nd // 2] = big[:-1] + b"!"   # same length, last byte differs
        docs[nd // 2 + 1] = big[:-1]      # a proper prefix
    return docs


def row_lists(ids, seed):
    rng = np.random.default_rng(seed)
    n = len(ids)
    yield ids
    yield ids[rng.permutation(n)[: max(3, n // 50)]]
    strangers = np.array([I64_MIN, I64_MAX, int(ids.max()) + 1, int(ids.min()) - 1], dtype=np.int64)
    mixed = np.concatenate([ids[: n // 2], ids[: n // 5], strangers, ids[n // 3:]])
    yield mixed[rng.permutation(len(mixed))]
    yield strangers
    yield np.empty(0, dtype=np.int64)


@pytest.mark.parametrize("ascending", [True, False])
@pytest.mark.parametrize("width", ["u32", "u64", "packed40"])
def test_string_cluster_entry_widths(width, ascending):
    # sizes as in test_packed_suffix_array_storage: 40000 tiny documents (16 bits) + one of 70000 bytes (17 bits) = 8-byte entries
    if width == "u32":
        docs, opts = pooled_docs(5000, seed=1), {}
    else:
        docs, opts = pooled_docs(40000, seed=2, long_doc=70000), ({"pack_sa": 0} if width == "u64" else {})
    nd = len(docs)
    ids = np.arange(nd, dtype=np.int64) * (1 << 33) - (1 << 40)
    if not ascending:
        ids = ids[np.random.default_rng(9).permutation(nd)]
    g = build_strings(docs, ids, **opts)
    assert g.sa_width == (4 if width == "u32" else 8) and g.stat("sa_packed") == (1 if width == "packed40" else 0)
    store = dict(zip(ids.tolist(), docs))
    for rows in row_lists(ids, seed=4):
        check_strings(g, store, rows)
    assert g.stat("cluster_classes") == len(set(docs))
    assert g.stat("cluster_table_bytes") >= 4 * nd + 4 * len(set(docs))
    g.close()


def test_unbuilt_index_has_no_groups():
    g = capi.GpuStringIndex(device=0)
    values, counts, reps, missing = g.cluster(np.array([1, 2, 2], dtype=np.int64))
    assert (values, len(counts), len(reps), missing) == ([], 0, 0, 3)
    g.add(1, b"x")
    assert g.cluster(np.array([1], dtype=np.int64))[3] == 1
    g.close()


def test_only_empty_documents():
    ids = np.array([5, 3, 9], dtype=np.int64)
    g = build_strings([b"", b"", b""], ids)
    check_strings(g, dict(zip(ids.tolist(), [b"", b"", b""])), np.array([9, 3, 3, 4], dtype=np.int64))
    g.close()


def _utf8_docs(nd, seed):
    rng = np.random.default_rng(seed)
    words = ["café", "naïve", "über", "日本語", "coffee", "db", "Ω", "ñandú", "zebra", "apple", "éclair", "東京", "a", ""]
    pool = ["".join(words[int(k)] for k in rng.integers(0, len(words), int(rng.integers(0, 4)))) for _ in range(400)]
    return [pool[int(k)].encode() for k in rng.integers(0, len(pool), nd)]


def _byte_docs(nd, seed):
    rng = np.random.default_rng(seed)
    pool = [bytes(W.random_bytes(int(rng.integers(0, 5)), seed * 100 + k, 0x00, 0xFF)) for k in range(3000)]
    pool += [bytes([b]) for b in (0x00, 0x7F, 0x80, 0xFF)] + [bytes([0x7F, 0x80]), bytes([0x80, 0x7F]), bytes([0xFF, 0x00])]
    return [pool[int(k)] for k in rng.integers(0, len(pool), nd)]


@pytest.mark.parametrize("compat", [1, 0])
@pytest.mark.parametrize("text", ["utf8", "bytes"])
def test_string_cluster_high_bytes_keep_std_string_order(text, compat):
    nd = 60000
    docs = _utf8_docs(nd, 31) if text == "utf8" else _byte_docs(nd, 32)
    ids = np.arange(nd, dtype=np.int64) + 10 ** 12
    g = build_strings(docs, ids, reference_compat=compat)
    if compat:
        # otherwise the test shows nothing: the array really is in the reference's order, not in std::string's
        assert g.stat("compat_rotations") > 0
        assert g.verify()["inversions"] > 0
    store = dict(zip(ids.tolist(), docs))
    for rows in row_lists(ids, seed=6):
        check_strings(g, store, rows)
    assert g.stat("cluster_resorted") == compat
    g.close()


def test_class_table_follows_rebuild_load_and_add(tmp_path):
    docs = pooled_docs(3000, seed=40)
    ids = np.arange(3000, dtype=np.int64) * 7
    g = build_strings(docs, ids)
    store = dict(zip(ids.tolist(), docs))
    check_strings(g, store, ids)
    assert g.stat("cluster_table_bytes") > 0
    # cdb_add + rebuild: new documents, one of them a new class, one joining an old class
    g.add(10 ** 9, b"brand new")
    g.add(10 ** 9 + 1, b"ab")
    check_strings(g, store, np.append(ids, [10 ** 9, 10 ** 9 + 1]))      # not built yet: the two are missing
    g.build()
    assert g.stat("cluster_table_bytes") == 0                             # the table went with the old array
    store[10 ** 9], store[10 ** 9 + 1] = b"brand new", b"ab"
    ids2 = np.append(ids, [10 ** 9, 10 ** 9 + 1])
    check_strings(g, store, ids2)
    # cdb_load into a handle that holds other documents (and their class table)
    path = os.path.join(str(tmp_path), "ix.cdb")
    g.save(path)
    docs3 = pooled_docs(500, seed=41, lo=0x70, hi=0x74)
    ids3 = np.arange(500, dtype=np.int64)
    h = build_strings(docs3, ids3)
    check_strings(h, dict(zip(ids3.tolist(), docs3)), ids3)
    h.load(path)
    assert h.stat("cluster_table_bytes") == 0
    check_strings(h, store, ids2)
    check_strings(h, store, ids3)                                         # (ids of the old column: whatever the new one holds)
    # a plain rebuild over different text under the same ids
    k = capi.GpuStringIndex(device=0)
    for i, d in zip(ids3.tolist(), docs3):
        k.add(i, d)
    k.build()
    check_strings(k, dict(zip(ids3.tolist(), docs3)), ids3)
    k.close()
    g.close()
    h.close()


def test_eight_threads_cluster_on_one_handle():
    docs = pooled_docs(20000, seed=50)
    ids = np.random.default_rng(51).permutation(np.arange(20000, dtype=np.int64) * 11 - 5000)
    g = build_strings(docs, ids)
    store = dict(zip(ids.tolist(), docs))
    assert g.stat("cluster_table_bytes") == 0                             # the first thread in makes the table
    lists = [ids[np.random.default_rng(60 + t).permutation(20000)[: 500 + 2000 * t]] for t in range(8)]
    expect = [string_model(store, rows) for rows in lists]
    got, errors = [None] * 8, []
    start = threading.Barrier(8)

    def work(t):
        try:
            start.wait()
            for _ in range(3):
                got[t] = g.cluster(lists[t])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(8):
        values, counts, reps, missing = got[t]
        assert (values, counts.tolist(), reps.tolist(), missing) == expect[t]
    g.close()


def test_midsize_string_column_multi_block_paths():
    # 256 MiB: 2^18 documents of 1 KiB drawn from 10^4 distinct ones
    nd, dl, npool = 1 << 18, 1024, 10 ** 4
    rng = np.random.default_rng(70)
    pool = rng.integers(0x61, 0x7B, (npool, dl), dtype=np.uint8)
    pick = rng.integers(0, npool, nd)
    blob = pool[pick].reshape(-1)
    ds = np.arange(nd + 1, dtype=np.uint64) * dl
    ids = np.arange(nd, dtype=np.int64) * 3 + 9
    g = capi.GpuStringIndex(device=0)
    g.build_view(ids, blob, ds)
    rank = np.empty(npool, dtype=np.int64)
    rank[np.argsort(pool.view("S%d" % dl).ravel(), kind="stable")] = np.arange(npool)   # std::string order of the pool
    assert len(np.unique(pool.view("S%d" % dl).ravel())) == npool
    sorted_pool = pool[np.argsort(rank)]
    for frac in (1.0, 0.02):
        sel = np.flatnonzero(rng.random(nd) < frac)
        rows = ids[sel][rng.permutation(len(sel))]
        ur, first, uc = np.unique(rank[pick[sel]], return_index=True, return_counts=True)
        values, counts, reps, missing = g.cluster(rows)
        assert missing == 0 and np.array_equal(counts, uc) and np.array_equal(reps, ids[sel][first])
        assert values == [sorted_pool[r].tobytes() for r in ur]
    assert g.stat("cluster_classes") == npool
    print("cluster_prepare_ms", g.stat("cluster_prepare_ms"), "cluster_ms", g.stat("cluster_ms"), "build_ms", g.stat("build_ms"))
    g.close()


def test_class_table_goes_with_an_array_the_order_proof_repairs():
    """The order proof behind a build (self_check = 3, the default) may find the published array damaged and replace it under the
    handle's lock.  A class table made from the damaged array (equal documents are no longer neighbours in it: a class splits and
    the same string shows up as two groups) must go with that array.  Damage = the test hook of tests/test_gpu_proof.py, aimed at
    two neighbouring offset-0 entries of DIFFERENT documents."""
    nd, npool = 250000, 2000
    rng = np.random.default_rng(80)
    pool = [bytes(W.random_bytes(int(rng.integers(40, 90)), 8000 + k, 0x61, 0x64)) for k in range(npool)]
    pick = rng.integers(0, npool, nd)
    docs = [pool[int(k)] for k in pick]
    ids = np.arange(nd, dtype=np.int64) * 2 + 7
    g = build_strings(docs, ids)
    assert g.proof_wait(60_000) == 2
    store = dict(zip(ids.tolist(), docs))
    rows = ids[rng.permutation(nd)]
    expect = string_model(store, rows)
    sa = g.sa().astype(np.uint64)
    off0 = (sa >> np.uint64(g.bits)) == 0
    doc = (sa & np.uint64(g.mask)).astype(np.int64)
    both = off0[:-1] & off0[1:] & (pick[doc[:-1]] != pick[doc[1:]])
    k = int(np.flatnonzero(both)[len(np.flatnonzero(both)) // 2])    # entries k, k + 1: whole documents of different text
    assert k > 0
    g.set_option("debug_damage_after_build", k)
    g.build()
    first = g.cluster(rows)                                          # at once: most likely still the damaged array
    # (the repair waits for the handle's lock while this call holds it; whether the call came first shows in its answer: a split
    #  class makes the groups differ from the model)
    saw_damage = (first[0], first[1].tolist()) != (expect[0], expect[1])
    assert g.proof_wait(60_000) == 3 and g.stat("self_check_fallbacks") == 1
    print("clustered the damaged array:", saw_damage, "groups then:", len(first[0]), "model:", len(expect[0]))
    if saw_damage:
        assert g.stat("cluster_table_bytes") == 0                    # the table went with the damaged array
    values, counts, reps, missing = g.cluster(rows)
    assert (values, counts.tolist(), reps.tolist(), missing) == expect
    assert g.stat("cluster_classes") == len(set(docs))
    check_strings(g, store, ids)
    g.close()
