"""Documents appended to a built index on the device (cdb_append, capi.GpuStringIndex.append).  The yardstick is always the
same: a FRESH handle built over the old documents followed by the new ones.  The appended-to handle must agree with it on the
layout, on the suffix array element for element, on queries, must pass the structural checks and the order proof, and where it
kept its search keys they must be the keys of its suffixes (verify_keys)."""
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


def append(g, ids, docs):
    blob, ds = pack(docs)
    return g.append(np.asarray(ids, dtype=np.int64), blob, ds)


def patterns(docs, seed=1, extra=()):
    """substrings that occur, a few that cannot (byte 0x01 is in no corpus here), and single bytes"""
    rng = np.random.default_rng(seed)
    pats = [b"\x01", b"a\x01", b"a", b"ab"] + list(extra)
    nonempty = [d for d in docs if d]
    for _ in range(60):
        if not nonempty:
            break
        d = nonempty[int(rng.integers(len(nonempty)))]
        a = int(rng.integers(len(d)))
        pats.append(d[a:a + 1 + int(rng.integers(6))])
    return pack(pats), pats


def assert_same(g, f, docs, lone=None, sorted_=True, extra=()):
    """g (appended to) against f (fresh over old + new); sorted_=False: the array is in the reference's order, where
    cdb_debug_verify's unsigned comparison does not apply (verify_reference is asked instead)"""
    assert (g.size, g.bits, g.mask, g.sa_width) == (f.size, f.bits, f.mask, f.sa_width)
    assert np.array_equal(g.sa(), f.sa())
    (pb, po), pats = patterns(docs, extra=extra)
    a, b = g.query_batch(pb, po), f.query_batch(pb, po)
    assert a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    for kw in ([lone] if lone else pats[3:8] + list(extra)):
        assert g.query(kw) == f.query(kw), kw
    if g.sa_width:
        v = g.verify()
        assert v["invalid_entries"] == 0 and v["entry_sum"] == v["expected_entry_sum"]
        if sorted_:
            assert v["inversions"] == v["tie_violations"] == 0
        else:
            assert g.verify_reference()["violations"] == 0
        assert g.proof_wait() == 2
        assert g.verify_keys()["mismatches"] == 0


def append_and_compare(ids, docs, new_ids, new_docs, sorted_=True, **opts):
    g = build(ids, docs, **opts)
    assert append(g, new_ids, new_docs) == len(new_ids)
    f = build(list(ids) + list(new_ids), list(docs) + list(new_docs), **opts)
    assert_same(g, f, list(docs) + list(new_docs), sorted_=sorted_)
    return g, f


CORPUS_A_IDS = [10, 11, 12, 13, 14, 15]
CORPUS_A = [b"abracadabra", b"", b"banana", b"banana", b"abra", b"cadabra banana"]   # empty, identical twins, a prefix of another

SMALL = {
    "twin_of_old": [b"banana"],                                  # ties go old first
    "two_new_twins": [b"nabana", b"nabana"],
    "prefixes": [b"abr", b"abracadabra banana"],                 # a proper prefix of an old document; an old one as a prefix of a new one
    "empty_only": [b"", b""],
    "one_byte": [b"n"],
    "below_all": [b"\x02\x03\x02", b"\x03"],                     # every byte sorts below every old byte
    "above_all": [b"~}~", b"}}"],                                # ... above
}


def recipe_b(seed, ndocs):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 4, size=int(rng.integers(0, 201)), dtype=np.uint8) + ord("a")) for _ in range(ndocs)]


@pytest.fixture(scope="module")
def corpus_b():
    return list(range(1000, 4000)), recipe_b(7, 3000)


def docs_of(blob, ds):
    return [bytes(blob[int(ds[d]):int(ds[d + 1])]) for d in range(len(ds) - 1)]


# ---- 1. small corpus ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(SMALL))
def test_small_corpus_equals_fresh_build(which):
    new = SMALL[which]
    g, _ = append_and_compare(CORPUS_A_IDS, CORPUS_A, list(range(100, 100 + len(new))), new)
    assert g.stat("appends") == 1 and g.stat("append_merges") == 1 and g.stat("append_rebuilds") == 0


# ---- 2. many tiles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 37, 600, 5000])
def test_many_tiles_equal_fresh_build(corpus_b, count):
    ids, docs = corpus_b
    new = recipe_b(100 + count, count)
    g, _ = append_and_compare(ids, docs, list(range(10000, 10000 + count)), new)
    assert g.stat("appends") == 1 and g.stat("append_merges") == 1 and g.stat("append_rebuilds") == 0
    assert g.stat("append_docs") == count and g.stat("append_bytes") == sum(len(d) for d in new)


# ---- 2b. merged lengths on the edges of a round (256 slots) and of a tile (4096) ------------------------------------------------
def split(total, parts, rng):
    """`parts` lengths >= 0 that sum to `total`"""
    cuts = np.sort(rng.integers(0, total + 1, size=parts - 1))
    return [int(x) for x in np.diff(np.concatenate([[0], cuts, [total]]))]


@pytest.mark.parametrize("where", ["below", "above"])
@pytest.mark.parametrize("total", [255, 256, 257, 4095, 4096, 4097, 8192])
def test_round_and_tile_edges_equal_fresh_build(total, where):
    # every new byte sorts below (above) every old byte: all new entries take the first (last) slots of the merged array
    rng = np.random.default_rng(total)
    m = total // 4
    lo = 0x02 if where == "below" else ord("}")
    docs = [bytes(rng.integers(0, 4, size=k, dtype=np.uint8) + ord("a")) for k in split(total - m, 12, rng)]
    new = [bytes(rng.integers(0, 2, size=k, dtype=np.uint8) + lo) for k in split(m, 4, rng)]
    g, f = append_and_compare(list(range(100, 112)), docs, list(range(500, 504)), new)
    assert (f.size, g.sa_width) == (total, 4) and g.stat("append_merges") == 1
    new_slots = np.flatnonzero((g.sa().astype(np.uint64) & np.uint64(g.mask)) >= 12)
    assert np.array_equal(new_slots, np.arange(m) + (0 if where == "below" else total - m))


# ---- 3. layout growth ----------------------------------------------------------------------------------------------------
def _edge(name):
    rng = np.random.default_rng(3)
    small = lambda n, m: [bytes(r) for r in rng.integers(0, 3, size=(n, m), dtype=np.uint8) + np.uint8(ord("a"))]  # noqa: E731
    long_doc = lambda m: bytes(rng.integers(0, 3, size=m, dtype=np.uint8) + ord("a"))  # noqa: E731
    if name == "doc_bits":          # 60 -> 70 documents: the document field gains a bit
        return small(60, 9), small(10, 9), lambda a, b: a[0] == 6 and b[0] == 7
    if name == "offset_bits":       # a new longest document: the offset field gains bits
        return small(50, 9), [long_doc(300)] + small(2, 9), lambda a, b: b[3] > a[3] and a[0] == b[0]
    if name == "width_4_to_8":      # 70 000 documents of 8 bytes (17 + 4 bits), then one of 40 000 bytes: 17 + 16 bits
        return small(70000, 8), [long_doc(40000)], lambda a, b: a[2] == 4 and b[2] == 8
    return small(70000, 8) + [long_doc(40000)], small(40, 8) + [long_doc(500)], lambda a, b: a[2] == 8 and b[2] == 8   # "width_8_stays"


@pytest.mark.parametrize("name,opts", [
    ("doc_bits", dict(pack_sa=1)), ("doc_bits", dict(pack_sa=0)),
    ("offset_bits", dict(pack_sa=1)), ("offset_bits", dict(pack_sa=0)),
    ("width_4_to_8", dict(pack_sa=1)), ("width_4_to_8", dict(pack_sa=0)), ("width_4_to_8", dict(pack_sa=1, force_big_path=1)),
    ("width_8_stays", dict(pack_sa=1)), ("width_8_stays", dict(pack_sa=0)),
])
def test_layout_growth(name, opts):
    # storage forms met as (source -> destination): u32 -> u32 (the first four), u32 -> packed, u32 -> u64 (width_4_to_8),
    # packed -> packed, u64 -> u64 (width_8_stays)
    docs, new, crossed = _edge(name)
    both = docs + new
    before = capi.layout_rule(len(docs), max(len(d) for d in docs))
    after = capi.layout_rule(len(both), max(len(d) for d in both))
    assert crossed(before, after), (before, after)
    g = build(list(range(len(docs))), docs, **opts)
    assert g.stat("sa_packed") == (1 if before[2] == 8 and opts.get("pack_sa") else 0)
    assert append(g, list(range(len(docs), len(both))), new) == len(new)
    assert g.stat("append_merges") == 1
    f = build(list(range(len(both))), both, **opts)
    assert g.stat("sa_packed") == f.stat("sa_packed") == (1 if after[2] == 8 and opts.get("pack_sa") else 0)
    assert_same(g, f, both[:1000] + new)


# ---- 4. paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat,old_hi,new_hi,forced,path", [
    (1, 0x7E, 0x7E, 0, "append_merges"),
    (0, 0xFF, 0xFF, 0, "append_merges"),
    (1, 0x7E, 0xFF, 0, "append_rebuilds"),
    (1, 0xFF, 0x7E, 0, "append_rebuilds"),
    (1, 0x7E, 0x7E, 2, "append_rebuilds"),
])
def test_paths(compat, old_hi, new_hi, forced, path):
    docs = docs_of(*W.ascii_corpus(300, 64, seed=3, lo=0x02, hi=old_hi))
    new = docs_of(*W.ascii_corpus(40, 64, seed=4, lo=0x02, hi=new_hi))
    in_reference_order = bool(compat and max(old_hi, new_hi) > 0x7F)
    g, f = append_and_compare(list(range(300)), docs, list(range(300, 340)), new, sorted_=not in_reference_order,
                              reference_compat=compat, debug_append_path=forced)
    assert g.stat(path) == 1 and g.stat("appends") == 1
    assert g.stat("append_rebuilds") + g.stat("append_merges") == 1
    if in_reference_order:
        assert g.verify_reference()["violations"] == 0
    if forced:   # ... and the forced rebuild equals the merge
        h = build(list(range(300)), docs, reference_compat=compat)
        append(h, list(range(300, 340)), new)
        assert h.stat("append_merges") == 1 and np.array_equal(h.sa(), g.sa())


# ---- 5. keys ---------------------------------------------------------------------------------------------------------------
def test_keys_are_kept_inside_the_old_alphabet(corpus_b):
    ids, docs = corpus_b
    ids, docs = ids[:800], docs[:800]
    g = build(ids, docs)
    ks = g.stat("key_symbols")
    plain = g.verify_keys()
    assert ks > 0 and plain["checked"] == g.size and plain["mismatches"] == 0     # (a plain build's keys are clean)
    new = recipe_b(55, 90)
    append(g, list(range(9000, 9090)), new)
    assert g.stat("append_keys_kept") == 1 and g.stat("key_symbols") == ks
    vk = g.verify_keys()
    assert vk["checked"] == g.size and vk["mismatches"] == 0
    assert_same(g, build(ids + list(range(9000, 9090)), docs + new), docs + new)
    # ... and after a removal
    assert g.remove(ids[3::5])[1] == 0
    vk = g.verify_keys()
    assert vk["checked"] == g.size and vk["mismatches"] == 0


def test_a_byte_the_old_text_never_held_drops_the_keys(corpus_b):
    ids, docs = corpus_b
    ids, docs = ids[:800], docs[:800]
    g = build(ids, docs)
    assert g.verify_keys()["checked"] == g.size
    new = [b"abzab", b"z", b"abcd"]
    append(g, [9000, 9001, 9002], new)
    assert g.stat("append_keys_kept") == 0 and g.verify_keys()["checked"] == 0
    assert g.query(b"z") == [(9000, 1), (9001, 1)] and g.query(b"bza") == [(9000, 1)]
    pb, po = pack([b"z", b"abz", b"abcd"])
    rp, rids, _, _ = g.query_batch(pb, po)
    assert list(rids[int(rp[0]):int(rp[1])]) == [9000, 9001] and list(rids[int(rp[1]):int(rp[2])]) == [9000]
    old_kw = docs[0][:5]
    assert g.query(old_kw) and ids[0] in [i for i, _ in g.query(old_kw)]
    assert_same(g, build(ids + [9000, 9001, 9002], docs + new), docs + new, extra=[b"z", b"zab"])


# ---- 6. state that rides along ------------------------------------------------------------------------------------------
def test_state_that_rides_along(corpus_b, tmp_path):
    ids, docs = corpus_b
    ids, docs = ids[:800], list(docs[:800])
    docs[5] = docs[9] = b"twin document"
    new_ids, new = list(range(9000, 9060)), recipe_b(21, 60)
    new[7] = b"twin document"
    g = build(ids, docs)
    append(g, new_ids, new)
    all_ids, all_docs = ids + new_ids, docs + new
    f = build(all_ids, all_docs)
    # cluster and render answer for old and new ids
    rows = np.array(ids[:100] + new_ids + [99999], dtype=np.int64)
    a, b = g.cluster(rows), f.cluster(rows)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] == 1
    found, texts, _, missing = g.render_rows([new_ids[7], ids[8], 77777], [b"ab"])
    assert list(found) == [True, True, False] and missing == 1 and texts[0] == b"twin document"
    assert g.render_rows([new_ids[7], ids[8], 77777], [b"ab"])[1:] == f.render_rows([new_ids[7], ids[8], 77777], [b"ab"])[1:]
    # save, load into a new handle
    path = str(tmp_path / "appended.idx")
    g.save(path)
    h = capi.GpuStringIndex(device=0)
    h.load(path)
    assert_same(h, f, all_docs)
    # two appends in a row = one append of both
    more_ids, more = list(range(9100, 9130)), recipe_b(22, 30)
    append(g, more_ids, more)
    u = build(ids, docs)
    append(u, new_ids + more_ids, new + more)
    assert g.stat("appends") == 2 and u.stat("appends") == 1
    assert_same(g, u, all_docs + more)
    # append then remove, remove then append
    gone = ids[9::4] + new_ids[::3]
    assert g.remove(gone) == (len(gone), 0)
    keep = [k for k, i in enumerate(all_ids + more_ids) if i not in set(gone)]
    kids, kdocs = [(all_ids + more_ids)[k] for k in keep], [(all_docs + more)[k] for k in keep]
    assert_same(g, build(kids, kdocs), kdocs)
    late_ids, late = [9500, 9501], [b"abcabc fresh", b"banana"]
    append(g, late_ids, late)
    assert_same(g, build(kids + late_ids, kdocs + late), kdocs + late)
    # add then build
    g.add(9600, b"dcba added the old way")
    g.build()
    final_docs = kdocs + late + [b"dcba added the old way"]
    assert_same(g, build(kids + late_ids + [9600], final_docs), final_docs)


# ---- 7. borrowed text ---------------------------------------------------------------------------------------------------
def test_borrowed_text_is_left_behind(corpus_b):
    import torch
    ids, docs = corpus_b
    ids, docs = ids[:500], docs[:500]
    blob, ds = pack(docs)
    t = torch.from_numpy(np.concatenate([blob, np.zeros(256, dtype=np.uint8)])).cuda()
    g = capi.GpuStringIndex(device=0)
    g.build_device(t.data_ptr(), ds, np.asarray(ids, dtype=np.int64))
    new_ids, new = list(range(9000, 9040)), recipe_b(31, 40)
    assert append(g, new_ids, new) == 40
    t.zero_()            # (a handle that still read the caller's buffer would now answer from zeros)
    torch.cuda.synchronize()
    del t
    assert_same(g, build(ids + new_ids, docs + new), docs + new)


# ---- 8. edges and refusals -----------------------------------------------------------------------------------------------
def test_no_documents_change_nothing():
    g = build(CORPUS_A_IDS, CORPUS_A)
    before = g.sa()
    assert append(g, [], []) == 0
    assert np.array_equal(g.sa(), before) and g.stat("appends") == 0


def test_never_built_handle_is_built():
    g = capi.GpuStringIndex(device=0)
    assert append(g, CORPUS_A_IDS, CORPUS_A) == len(CORPUS_A)
    assert_same(g, build(CORPUS_A_IDS, CORPUS_A), CORPUS_A)
    e = build([], [])   # built over nothing
    assert append(e, CORPUS_A_IDS, CORPUS_A) == len(CORPUS_A)
    assert_same(e, build(CORPUS_A_IDS, CORPUS_A), CORPUS_A)


def test_pending_additions_are_refused():
    g = build(CORPUS_A_IDS, CORPUS_A)
    before = g.sa()
    g.add(99, b"late")
    with pytest.raises(RuntimeError, match="append: documents were added since the last build"):
        append(g, [100], [b"banana"])
    assert np.array_equal(g.sa(), before) and g.query(b"banana") == [(12, 1), (13, 1), (15, 1)]


def test_failed_merge_leaves_the_old_index_serving():
    g = build(CORPUS_A_IDS, CORPUS_A)
    before = g.sa()
    g.set_option("debug_fail_build", 1)
    with pytest.raises(RuntimeError, match="build failure requested"):
        append(g, [100], [b"banana"])
    assert np.array_equal(g.sa(), before) and g.query(b"banana") == [(12, 1), (13, 1), (15, 1)]
    assert g.stat("appends") == 0


def test_failed_rebuild_leaves_an_unbuilt_handle():
    # (corpus and keyword of test_failed_build_leaves_index_unbuilt: in the reference's order a lone keyword follows the reference's
    #  probe sequence, which does not find every substring of text with bytes >= 0x80 — this one it finds)
    blob, ds = W.ascii_corpus(300, 64, seed=3, lo=0x00, hi=0xFF)
    g = build(list(range(300)), docs_of(blob, ds))
    kw = bytes(blob[:2])
    assert g.query(kw)
    g.set_option("debug_fail_build", 1)
    with pytest.raises(RuntimeError, match="build failure requested"):
        append(g, [1000], [b"one more"])
    assert g.sa_width == 0 and g.query(kw) == []


# ---- 9. concurrency -----------------------------------------------------------------------------------------------------
def test_queries_beside_an_append_see_before_or_after():
    blob, ds = W.ascii_corpus(2000, 128, seed=3)
    docs = docs_of(blob, ds)
    old_ids, old, new_ids, new = list(range(1000)), docs[:1000], list(range(1000, 2000)), docs[1000:]
    pb, po = W.sample_patterns(blob, ds, 64, 2, 6, seed=10)
    kws = [bytes(pb[int(po[j]):int(po[j + 1])]) for j in range(64)]
    g = build(old_ids, old)
    before = [g.query(k) for k in kws]
    f = build(old_ids + new_ids, docs)
    after = [f.query(k) for k in kws]
    assert before != after
    errs = []

    def ask(t):
        try:
            for j in range(t, 64, 2):
                assert g.query(kws[j]) in (before[j], after[j]), kws[j]
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def join():
        try:
            assert append(g, new_ids, new) == len(new_ids)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=ask, args=(0,)), threading.Thread(target=ask, args=(1,)), threading.Thread(target=join)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs
    assert [g.query(k) for k in kws] == after
