"""Documents removed from a built index on the device (cdb_remove / cdb_column_remove, capi.GpuStringIndex.remove /
GpuColumn.remove).  The yardstick is always the same: a FRESH handle built over the surviving documents in their original
order.  The removed-from handle must agree with it on the layout, on the suffix array element for element, on queries, and
must pass the structural checks and the order proof."""
import threading

import numpy as np
import pytest

from coffeedb_amd import capi, workloads as W

pytestmark = pytest.mark.gpu


# ---- helpers -----------------------------------------------------------------------------------------------------------
def pack(docs):
    blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    return blob, ds


def build(ids, docs, **opts):
    g = capi.GpuStringIndex(device=0)
    for k, v in opts.items():
        g.set_option(k, v)
    blob, ds = pack(docs)
    g.add_bulk(np.asarray(ids, dtype=np.int64), blob, ds)
    g.build()
    return g


def survivors(ids, docs, gone):
    gone = set(int(x) for x in gone)
    keep = [k for k, i in enumerate(ids) if int(i) not in gone]
    return [ids[k] for k in keep], [docs[k] for k in keep]


def expected_counts(ids, gone):
    held = set(int(i) for i in ids)
    return len(held & set(int(x) for x in gone)), sum(1 for x in gone if int(x) not in held)


def patterns(docs, seed=1):
    """substrings that occur, a few that cannot (byte 0x01 is in no corpus here), and single bytes"""
    rng = np.random.default_rng(seed)
    pats = [b"\x01", b"a\x01", b"a", b"ab"]
    nonempty = [d for d in docs if d]
    for _ in range(60):
        if not nonempty:
            break
        d = nonempty[int(rng.integers(len(nonempty)))]
        a = int(rng.integers(len(d)))
        pats.append(d[a:a + 1 + int(rng.integers(6))])
    return pack(pats), pats


def assert_same(g, f, docs, lone=None, sorted_=True):
    """g (removed from) against f (fresh over the survivors); sorted_=False: the array is in the reference's order, where
    cdb_debug_verify's unsigned comparison does not apply (verify_reference is asked instead)"""
    assert (g.size, g.bits, g.mask, g.sa_width) == (f.size, f.bits, f.mask, f.sa_width)
    assert np.array_equal(g.sa(), f.sa())
    (pb, po), pats = patterns(docs)
    a, b = g.query_batch(pb, po), f.query_batch(pb, po)
    assert a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    for kw in ([lone] if lone else pats[3:8]):
        assert g.query(kw) == f.query(kw), kw
    if g.sa_width:
        v = g.verify()
        assert v["invalid_entries"] == 0 and v["entry_sum"] == v["expected_entry_sum"]
        if sorted_:
            assert v["inversions"] == v["tie_violations"] == 0
        else:
            assert g.verify_reference()["violations"] == 0
        assert g.proof_wait() == 2


def remove_and_compare(ids, docs, gone, sorted_=True, **opts):
    g = build(ids, docs, **opts)
    removed, missing = g.remove(gone)
    assert (removed, missing) == expected_counts(ids, gone)
    kids, kdocs = survivors(ids, docs, gone)
    f = build(kids, kdocs, **opts)
    assert_same(g, f, kdocs, sorted_=sorted_)
    return g, f


CORPUS_A_IDS = [10, 11, 12, 13, 14, 15]
CORPUS_A = [b"abracadabra", b"", b"banana", b"banana", b"abra", b"cadabra banana"]   # empty, identical twins, a prefix of another


@pytest.fixture(scope="module")
def corpus_b():
    rng = np.random.default_rng(7)
    docs = [bytes(rng.integers(0, 4, size=int(rng.integers(0, 201)), dtype=np.uint8) + ord("a")) for _ in range(3000)]
    return list(range(1000, 4000)), docs


def removal_sets(ids):
    return {
        "not_held": [ids[-1] + 77],
        "first": [ids[0]],
        "last": [ids[-1]],
        "every_second": ids[::2],
        "all_but_one": ids[:len(ids) // 2] + ids[len(ids) // 2 + 1:],
        "all": list(ids),
        "repeats": [ids[1], ids[1], ids[-1] + 5, ids[2], ids[-1] + 5, ids[1]],
    }


SETS = ["not_held", "first", "last", "every_second", "all_but_one", "all", "repeats"]


# ---- 1. equals a fresh build -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SETS)
def test_small_corpus_equals_fresh_build(which):
    remove_and_compare(CORPUS_A_IDS, CORPUS_A, removal_sets(CORPUS_A_IDS)[which])


@pytest.mark.parametrize("which", SETS)
def test_many_tiles_equal_fresh_build(corpus_b, which):
    ids, docs = corpus_b
    g, _ = remove_and_compare(ids, docs, removal_sets(ids)[which])
    if which != "not_held":
        assert g.stat("removes") == 1 and g.stat("remove_compactions") == 1 and g.stat("remove_rebuilds") == 0
        assert g.stat("remove_docs") == expected_counts(ids, removal_sets(ids)[which])[0]
    else:
        assert g.stat("removes") == 0


def test_empty_id_list_changes_nothing(corpus_b):
    ids, docs = corpus_b
    g = build(ids[:50], docs[:50])
    before = g.sa()
    assert g.remove([]) == (0, 0)
    assert np.array_equal(g.sa(), before)


# ---- 1b. array lengths on the edges of a round (256 entries) and of a tile (4096) ---------------------------------------------
def split(total, parts, rng):
    """`parts` lengths >= 0 that sum to `total`"""
    cuts = np.sort(rng.integers(0, total + 1, size=parts - 1))
    return [int(x) for x in np.diff(np.concatenate([[0], cuts, [total]]))]


EDGE_N = [255, 256, 257, 4095, 4096, 4097, 8192]
# (old length, which documents go, kept length): half and nearly all of every old length, and the kept length itself on a tile edge
EDGE_CASES = ([(n, "every_second", n // 2) for n in EDGE_N] + [(n, "last", n - 1 - n // 16) for n in EDGE_N] +
              [(8192, "last", 4097), (4097, "last", 4096), (8192, "every_second", 4097)])


@pytest.mark.parametrize("n,which,kept", EDGE_CASES)
def test_round_and_tile_edges_equal_fresh_build(n, which, kept):
    rng = np.random.default_rng(n * 3 + kept)
    if which == "every_second":   # documents 0, 2, 4, ... go
        lens = [x for pair in zip(split(n - kept, 8, rng), split(kept, 8, rng)) for x in pair]
    else:
        lens = split(kept, 15, rng) + [n - kept]
    docs = [bytes(rng.integers(0, 4, size=m, dtype=np.uint8) + ord("a")) for m in lens]
    ids = list(range(100, 100 + len(docs)))
    gone = ids[::2] if which == "every_second" else [ids[-1]]
    g, f = remove_and_compare(ids, docs, gone)
    assert (sum(lens), f.size, g.sa_width) == (n, kept, 4) and g.stat("remove_compactions") == 1


# ---- 2. layout edges ---------------------------------------------------------------------------------------------------
def _edge(name):
    rng = np.random.default_rng(3)
    small = lambda n, m: [bytes(r) for r in rng.integers(0, 3, size=(n, m), dtype=np.uint8) + np.uint8(ord("a"))]  # noqa: E731
    if name == "offset_bits":       # the longest document goes: fewer offset bits
        docs = small(50, 9) + [bytes(rng.integers(0, 3, size=300, dtype=np.uint8) + ord("a"))]
        ids = list(range(len(docs)))
        return ids, docs, [50], lambda a, b: a[3] > b[3]
    if name == "doc_bits":          # 70 -> 60 documents: the document field loses a bit
        docs = small(70, 9)
        ids = list(range(70))
        return ids, docs, list(range(5, 15)), lambda a, b: a[0] == 7 and b[0] == 6
    # 70 000 documents of 8 bytes + one of 40 000: 17 + 16 bits, 8-byte entries
    docs = small(70000, 8) + [bytes(rng.integers(0, 3, size=40000, dtype=np.uint8) + ord("a"))]
    ids = list(range(len(docs)))
    if name == "width_8_to_4":      # the long one goes: 17 + 4 bits, 4-byte entries
        return ids, docs, [70000], lambda a, b: a[2] == 8 and b[2] == 4
    return ids, docs, list(range(0, 3000, 3)), lambda a, b: a[2] == 8 and b[2] == 8    # "width_8_stays"


@pytest.mark.parametrize("name,opts", [
    ("offset_bits", dict(pack_sa=1)), ("offset_bits", dict(pack_sa=0)),
    ("doc_bits", dict(pack_sa=1)), ("doc_bits", dict(pack_sa=0)),
    ("width_8_to_4", dict(pack_sa=1)), ("width_8_to_4", dict(pack_sa=0)), ("width_8_to_4", dict(pack_sa=1, force_big_path=1)),
    ("width_8_stays", dict(pack_sa=1)), ("width_8_stays", dict(pack_sa=0)),
])
def test_layout_edges(name, opts):
    # storage forms met as (source -> destination): u32 -> u32 (the first two), packed -> u32, u64 -> u32 (width_8_to_4),
    # packed -> packed, u64 -> u64 (width_8_stays)
    ids, docs, gone, crossed = _edge(name)
    kids, kdocs = survivors(ids, docs, gone)
    before = capi.layout_rule(len(docs), max(len(d) for d in docs))
    after = capi.layout_rule(len(kdocs), max(len(d) for d in kdocs))
    assert crossed(before, after), (before, after)
    g = build(ids, docs, **opts)
    packed_before = g.stat("sa_packed")
    assert packed_before == (1 if before[2] == 8 and opts.get("pack_sa") else 0)
    assert g.remove(gone) == (len(gone), 0)
    f = build(kids, kdocs, **opts)
    assert g.stat("sa_packed") == f.stat("sa_packed") == (1 if after[2] == 8 and opts.get("pack_sa") else 0)
    assert_same(g, f, kdocs[:2000])


# ---- 3. both paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat,high,path", [(1, True, "remove_rebuilds"), (0, True, "remove_compactions"), (1, False, "remove_compactions")])
def test_both_paths(compat, high, path):
    blob, ds = W.ascii_corpus(300, 64, seed=3, lo=0x02, hi=0xFF if high else 0x7E)
    docs = [bytes(blob[int(ds[d]):int(ds[d + 1])]) for d in range(300)]
    ids = list(range(300))
    g, f = remove_and_compare(ids, docs, ids[3::7], sorted_=not (compat and high), reference_compat=compat)
    assert g.stat(path) == 1 and g.stat("removes") == 1
    assert g.stat("remove_rebuilds") + g.stat("remove_compactions") == 1
    if compat and high:
        assert g.verify_reference()["violations"] == 0


# ---- 4. state that rides along ------------------------------------------------------------------------------------------
def test_state_that_rides_along(corpus_b, tmp_path):
    ids, docs = corpus_b
    ids, docs = ids[:800], docs[:800]
    docs[5] = docs[9] = docs[700] = b"twin document"
    gone = ids[9::4]
    g = build(ids, docs)
    ks = g.stat("key_symbols")
    g.remove(gone)
    kids, kdocs = survivors(ids, docs, gone)
    f = build(kids, kdocs)
    # cluster
    rows = np.array(ids[:400] + [99999], dtype=np.int64)
    a, b = g.cluster(rows), f.cluster(rows)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    # render
    found, texts, _, missing = g.render_rows([ids[9], ids[8]], [b"ab"])
    assert list(found) == [False, True] and missing == 1 and texts[0] == b""
    # the keys were kept
    assert g.stat("key_symbols") == ks and ks > 0 and g.stat("remove_compactions") == 1
    # save, load into a new handle
    path = str(tmp_path / "removed.idx")
    g.save(path)
    h = capi.GpuStringIndex(device=0)
    h.load(path)
    assert_same(h, f, kdocs)
    # two removals in a row = one removal of the union
    more = kids[1::5]
    g.remove(more)
    kids2, kdocs2 = survivors(kids, kdocs, more)
    u = build(ids, docs)
    assert u.remove(list(gone) + list(more)) == (len(gone) + len(more), 0)
    assert_same(g, u, kdocs2)
    # add then build
    new_ids, new_docs = [500000, 500001], [b"abcabc fresh", b"banana"]
    for i, d in zip(new_ids, new_docs):
        g.add(i, d)
    g.build()
    f2 = build(kids2 + new_ids, kdocs2 + new_docs)
    assert_same(g, f2, kdocs2 + new_docs)


# ---- 5. borrowed text ---------------------------------------------------------------------------------------------------
def test_borrowed_text_is_left_behind(corpus_b):
    import torch
    ids, docs = corpus_b
    ids, docs = ids[:500], docs[:500]
    blob, ds = pack(docs)
    t = torch.from_numpy(np.concatenate([blob, np.zeros(256, dtype=np.uint8)])).cuda()
    g = capi.GpuStringIndex(device=0)
    g.build_device(t.data_ptr(), ds, np.asarray(ids, dtype=np.int64))
    gone = ids[::3]
    assert g.remove(gone) == (len(gone), 0)
    t.zero_()            # (a handle that still read the caller's buffer would now answer from zeros)
    torch.cuda.synchronize()
    del t
    kids, kdocs = survivors(ids, docs, gone)
    assert_same(g, build(kids, kdocs), kdocs)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_pending_additions_are_refused():
    g = build(CORPUS_A_IDS, CORPUS_A)
    before = g.sa()
    g.add(99, b"late")
    with pytest.raises(RuntimeError, match="remove: documents were added since the last build"):
        g.remove([10])
    assert np.array_equal(g.sa(), before) and g.query(b"banana") == [(12, 1), (13, 1), (15, 1)]


def test_never_built_handle_holds_no_id():
    g = capi.GpuStringIndex(device=0)
    assert g.remove([1, 2, 2]) == (0, 3)
    assert g.sa_width == 0


def test_failed_rebuild_leaves_an_unbuilt_handle():
    # (corpus and keyword of test_failed_build_leaves_index_unbuilt: in the reference's order a lone keyword follows the reference's
    #  probe sequence, which does not find every substring of text with bytes >= 0x80 — this one it finds)
    blob, ds = W.ascii_corpus(300, 64, seed=3, lo=0x00, hi=0xFF)
    docs = [bytes(blob[int(ds[d]):int(ds[d + 1])]) for d in range(300)]
    g = build(list(range(300)), docs)
    kw = bytes(blob[:2])
    assert g.query(kw)
    g.set_option("debug_fail_build", 1)
    with pytest.raises(RuntimeError, match="build failure requested"):
        g.remove([3])
    assert g.sa_width == 0 and g.query(kw) == []


# ---- 7. columns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bool", "int64", "double"])
def test_column_remove_equals_fresh_column(kind):
    rng = np.random.default_rng(11)
    n = 1000
    ids = rng.permutation(np.arange(5000, 5000 + n)).astype(np.int64)
    vals = {"bool": rng.integers(0, 2, n), "int64": rng.integers(-20, 20, n), "double": rng.integers(-20, 20, n) / 4.0}[kind]
    gone = list(ids[::3]) + [int(ids[3]), 1, 1, 2]
    c = capi.GpuColumn(kind, device=0)
    c.add_bulk(ids, vals)
    c.build()
    assert c.remove(gone) == (len(ids[::3]), 3)
    keep = ~np.isin(ids, ids[::3])
    f = capi.GpuColumn(kind, device=0)
    f.add_bulk(ids[keep], vals[keep])
    f.build()
    assert c.stat("rows") == f.stat("rows") == int(keep.sum())
    ranges = ["true", "false"] if kind == "bool" else ["[-inf,inf]", "[-3,2]", "(0,5]", "[100,200]", "[-5,-5]"]
    for r in ranges:
        assert c.query(r) == f.query(r), r
    assert np.array_equal(c.query_any(ranges[:2]), f.query_any(ranges[:2]))
    rows = np.concatenate([ids[:300], [1, 2]]).astype(np.int64)
    a, b = c.cluster(rows), f.cluster(rows)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert c.remove([]) == (0, 0) and c.remove([1]) == (0, 1)


# ---- 8. concurrency -----------------------------------------------------------------------------------------------------
def test_queries_beside_a_removal_see_before_or_after():
    blob, ds = W.ascii_corpus(2000, 128, seed=3)
    docs = [bytes(blob[int(ds[d]):int(ds[d + 1])]) for d in range(2000)]
    ids = list(range(2000))
    gone = ids[::2]
    pb, po = W.sample_patterns(blob, ds, 64, 2, 6, seed=10)
    kws = [bytes(pb[int(po[j]):int(po[j + 1])]) for j in range(64)]
    g = build(ids, docs)
    before = [g.query(k) for k in kws]
    f = build(*survivors(ids, docs, gone))
    after = [f.query(k) for k in kws]
    errs = []

    def ask(t):
        try:
            for j in range(t, 64, 2):
                assert g.query(kws[j]) in (before[j], after[j]), kws[j]
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def drop():
        try:
            assert g.remove(gone) == (len(gone), 0)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=ask, args=(0,)), threading.Thread(target=ask, args=(1,)), threading.Thread(target=drop)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs
    assert [g.query(k) for k in kws] == after
