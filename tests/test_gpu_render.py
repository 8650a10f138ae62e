"""A page of result rows rendered on the device (cdb_render_rows / cdb_shards_render_rows, capi.*.render_rows) against the
reference's highlighter restated here from database.cpp:58-90: ac_automaton::render walks a document, takes at every end
position the longest keyword ending there and merges it into a span list by the pop / extend / append rule; `left` goes before
every span's first byte and `right` after its last.  found, missing, text_ptr, text_blob, span_ptr, begin and end are all
compared for equality."""
import random
import threading

import numpy as np
import pytest

from coffeedb_amd import capi

pytestmark = pytest.mark.gpu


# ---- the model ---------------------------------------------------------------------------------------------------------
def model_render(text, keywords, left, right):
    """database.cpp:58-90.  Returns (spans [(begin, end_inclusive)], rendered bytes)."""
    lens = sorted({len(k) for k in keywords}, reverse=True)
    kws = set(keywords)
    spans = []
    for i in range(len(text)):
        length = 0   # length[node]: the longest keyword that ends at i
        for m in lens:
            if m <= i + 1 and text[i + 1 - m:i + 1] in kws:
                length = m
                break
        if length:
            begin = i - length + 1
            while spans and begin <= spans[-1][0]:
                spans.pop()
            if spans and begin <= spans[-1][1]:
                spans[-1][1] = i
            else:
                spans.append([begin, i])
    ret, it = bytearray(), 0
    for i in range(len(text)):
        if it < len(spans) and i == spans[it][0]:
            ret += left
        ret.append(text[i])
        if it < len(spans) and i == spans[it][1]:
            ret += right
            it += 1
    return [tuple(s) for s in spans], bytes(ret)


def model_page(store, page, keywords, left, right):
    found, missing, tp, sp, blob, beg, end = [], 0, [0], [0], bytearray(), [], []
    cache = {}
    for i in page:
        i = int(i)
        if i in store:
            if i not in cache:
                cache[i] = model_render(store[i], keywords, left, right)
            spans, txt = cache[i]
            blob += txt
            beg += [s[0] for s in spans]
            end += [s[1] for s in spans]
        else:
            missing += 1
        found.append(i in store)
        tp.append(len(blob))
        sp.append(len(beg))
    return found, missing, tp, bytes(blob), sp, beg, end


def check(ix, store, page, keywords, left=b"<b>", right=b"</b>"):
    r = ix.render_rows(page, keywords, left, right, raw=True)
    found, missing, tp, blob, sp, beg, end = model_page(store, page, keywords, left, right)
    assert r["found"].tolist() == found
    assert r["missing"] == missing
    assert r["span_ptr"].tolist() == sp
    assert r["begin"].tolist() == beg
    assert r["end"].tolist() == end
    assert r["nspans"] == len(beg)
    assert r["text_ptr"].tolist() == tp
    assert r["text_bytes"] == len(blob)
    assert r["text_blob"] == blob
    return r


def make_index(docs, ids=None, compat=None):
    ids = np.arange(len(docs), dtype=np.int64) * 3 + 7 if ids is None else np.asarray(ids, dtype=np.int64)
    ix = capi.GpuStringIndex()
    if compat is not None:
        ix.set_option("reference_compat", compat)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    blob = np.frombuffer(b"".join(docs) or b"\0", dtype=np.uint8)
    ix.add_bulk(ids, blob, ds)
    ix.build()
    return ix, {int(i): d for i, d in zip(ids, docs)}


# ---- 1. the reference's README vector ------------------------------------------------------------------------------------
def test_readme_vector():
    ix, store = make_index([b"3010103"])
    found, texts, spans, missing = ix.render_rows([7], [b"010"], b"<b>", b"</b>")
    assert texts == [b"3<b>01010</b>3"] and spans == [[(1, 5)]] and found.tolist() == [True] and missing == 0
    check(ix, store, [7], [b"010"])


# ---- 2. the merge rule on minimal strings --------------------------------------------------------------------------------
def test_merge_rule_minimal():
    docs = [b"abab", b"aaaa", b"abcd", b"", b"xab", b"cdy", b"", b"abc", b"a", b"zzabcabcdzz"]
    ix, store = make_index(docs)
    page = sorted(store)
    assert ix.render_rows([7], [b"ab"])[2] == [[(0, 1), (2, 3)]]          # adjacent occurrences stay apart
    assert ix.render_rows([10], [b"aa"])[2] == [[(0, 3)]]                  # overlapping ones fuse
    for kws in ([b"ab"], [b"aa"], [b"a", b"ab", b"abc"], [b"abc", b"bcd", b"d"], [b"abcd"], [b"abcde"], [b"abcd", b"abcdabcd"],
                [b"abcdy"], [b"bc"], [b"dx", b"bcd"]):
        for left, right in ((b"<b>", b"</b>"), (b"", b"]"), (b"[", b""), (b"", b"")):
            check(ix, store, page, kws, left, right)
    # "abcd" + "" + "xab": "dx" / "dxab" would only match across a document boundary
    assert ix.render_rows(page, [b"dx", b"dxab", b"bx", b"yabc"])[2] == [[] for _ in page]


# ---- 3. tile and wave edges ----------------------------------------------------------------------------------------------
def test_tile_edges_one_long_document():
    n = 3 * 4096 + 17
    doc = bytearray(b"." * n)
    for at in (4095, 4094, 8191, 8189, 0, n - 2, 4096 * 2 + 4090):   # occurrences straddling page positions 4095/4096 and 8191/8192
        doc[at:at + 2] = b"xy"
    doc[8189:8194] = b"qrstu"
    doc[4094:4097] = b"xyz"
    ix, store = make_index([bytes(doc)])
    check(ix, store, [7], [b"xy", b"xyz", b"qrstu", b"rs"])
    check(ix, store, [7, 7], [b"xy", b"."])   # the second copy starts at page position n: other tile phases


def test_one_span_across_tiles():
    ix, store = make_index([b"b", b"a" * 5000, b"ba"])
    r = check(ix, store, [10, 7, 10, 13], [b"aa"])
    assert r["begin"].tolist() == [0, 0] and r["end"].tolist() == [4999, 4999]


def test_many_short_documents_shuffled_page():
    rng = random.Random(5)
    docs = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(8))) for _ in range(2000)]
    ix, store = make_index(docs)
    page = [rng.choice([7 + 3 * rng.randrange(2000), 7 + 3 * rng.randrange(2000), 8 + 3 * rng.randrange(3000), -5]) for _ in range(3000)]
    check(ix, store, page, [b"ab", b"ba", b"bbb"])
    check(ix, store, sorted(store), [b"a"], b"", b"")


# ---- 4. fuzz ---------------------------------------------------------------------------------------------------------------
def test_fuzz():
    for group in range(5):
        rng = random.Random(1000 + group)
        alpha = b"ab" if group % 2 else b"abc"
        docs = [bytes(rng.choice(alpha) for _ in range(rng.randrange(301))) for _ in range(150)]
        ids = rng.sample(range(-500, 500), len(docs)) if group % 2 else None   # both id-table forms
        ix, store = make_index(docs, ids)
        have = sorted(store)
        for seed in range(10):
            rng = random.Random(group * 10 + seed)
            kws = [bytes(rng.choice(alpha) for _ in range(rng.randrange(1, 7))) for _ in range(rng.randrange(1, 9))]
            left = bytes(rng.randrange(256) for _ in range(rng.randrange(6)))
            right = bytes(rng.randrange(256) for _ in range(rng.randrange(6)))
            page = [rng.choice(have) if rng.random() < 0.85 else rng.randrange(-2000, 2000) for _ in range(rng.randrange(201))]
            check(ix, store, page, kws, left, right)
        ix.close()


# ---- 5. a keyword list beyond one LDS chunk --------------------------------------------------------------------------------
def test_keyword_list_beyond_one_chunk():
    rng = random.Random(9)
    long_kw = bytes(rng.choice(b"abcdefgh") for _ in range(5000))
    docs = [bytes(rng.choice(b"abcdefgh") for _ in range(rng.randrange(600, 1200))) for _ in range(30)]
    docs[17] = docs[17][:300] + long_kw + docs[17][300:]                  # planted once
    docs[18] = long_kw[:4999] + b"h" if long_kw[4999:] != b"h" else long_kw[:4999] + b"a"   # equal up to the last byte
    kws = [long_kw] + [bytes(rng.choice(b"abcdefgh") for _ in range(rng.randrange(3, 60))) for _ in range(299)]
    kws += [docs[3][10:300], docs[3][10:400]]                              # longer than what the LDS keeps of a keyword
    assert len(kws) > 256 and sum(map(len, kws)) > 8192
    ix, store = make_index(docs)
    r = check(ix, store, sorted(store), kws)
    assert any(e - b + 1 >= 5000 for b, e in zip(r["begin"].tolist(), r["end"].tolist()))


# ---- 6. bytes >= 0x80 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat", [1, 0])
def test_high_bytes(compat):
    rng = random.Random(3)
    docs = [bytes(rng.randrange(0x70, 0x91) for _ in range(rng.randrange(120))) for _ in range(300)]
    utf = "żółw ελληνικά 日本語 żółć naïve ".encode()
    docs += [b"".join(rng.choice([utf[:9], utf[9:28], utf[28:38], utf]) for _ in range(rng.randrange(6))) for _ in range(200)]
    ix, store = make_index(docs, compat=compat)
    page = rng.sample(sorted(store), 400)
    check(ix, store, page, [bytes([0x80]), bytes([0x7f, 0x80]), bytes([0x90, 0x70]), bytes([0x81, 0x82, 0x83])])
    check(ix, store, page, ["ół".encode(), "λλ".encode(), "日本".encode(), b"\xc5", "ï".encode()])
    assert ix.stat("cluster_prepare_ms") == 0   # the class table (a host sort under reference_compat) was not built


# ---- 7. second implementation ----------------------------------------------------------------------------------------------
def test_equals_query_spans_on_ascii():
    rng = random.Random(11)
    docs = [bytes(rng.choice(b"abcd") for _ in range(rng.randrange(100))) for _ in range(500)]
    ix, store = make_index(docs)
    kws = [b"ab", b"bcd", b"dd", b"abca"]
    by_id = dict(ix.query_spans(kws))
    page = sorted(store)
    _, _, spans, _ = ix.render_rows(page, kws)
    assert len(by_id) > 100
    for i, sp in zip(page, spans):
        assert sp == [(int(b), int(e)) for b, e in by_id.get(i, [])]


def test_reference_highlight_property():
    """test/test-highlight.py:53-60: disjoint keywords, rendered text == sequential replace(k, "<b>k</b>")."""
    rng = random.Random(12)
    alphabet = list("abcdefghijklmnopqrstuvwxyz")
    rng.shuffle(alphabet)
    kws = ["".join(alphabet[4 * k:4 * k + 4]).encode() for k in range(5)]
    docs = []
    for _ in range(200):
        d = b""
        while len(d) < 500:
            d += rng.choice(kws) if rng.random() < 0.3 else bytes([rng.choice(b"abcdefghijklmnopqrstuvwxyz")])
        docs.append(d[:500])
    ix, store = make_index(docs)
    page = sorted(store)
    _, texts, _, _ = ix.render_rows(page, kws, b"<b>", b"</b>")
    for i, t in zip(page, texts):
        want = store[i]
        for k in kws:
            want = want.replace(k, b"<b>" + k + b"</b>")
        # (neighbouring occurrences of different keywords stay apart in the reference too: adjacent spans do not fuse)
        assert t == want
    check(ix, store, page[:20], kws)


# ---- 8. life cycle ---------------------------------------------------------------------------------------------------------
def test_unbuilt_nokeywords_what_and_errors(tmp_path):
    ix = capi.GpuStringIndex()
    r = ix.render_rows([1, 2, 3], [b"a"], b"<", b">", raw=True)           # unbuilt: all rows missing
    assert r["found"].tolist() == [False] * 3 and r["missing"] == 3 and r["text_ptr"].tolist() == [0] * 4
    assert r["span_ptr"].tolist() == [0] * 4 and r["text_blob"] == b"" and r["nspans"] == 0
    ix.close()
    docs = [b"hello world", b"", b"low low"]
    ix, store = make_index(docs, ids=[30, 10, 20])                         # ids not ascending
    check(ix, store, [10, 20, 30, 40, 20], [])                             # nkw = 0: the plain documents
    assert ix.render_rows([30, 99], [], b"<", b">")[1] == [b"hello world", b""]
    check(ix, store, [], [b"lo"])                                          # nrows = 0
    r = ix.render_rows([20, 30], [b"lo"], b"<", b">", spans=False, raw=True)
    assert r["span_ptr"] is None and r["begin"] is None and r["text_blob"] == b"<lo>w <lo>whel<lo> world"
    r = ix.render_rows([20, 30], [b"lo"], b"<", b">", text=False, raw=True)
    assert r["text_ptr"] is None and r["text_blob"] is None and r["begin"].tolist() == [0, 4, 3] and r["end"].tolist() == [1, 5, 4]
    with pytest.raises(RuntimeError, match="Empty keywords are not allowed"):
        ix.render_rows([20], [b"lo", b""])
    assert ix.stat("render_page_bytes") == 18 and ix.stat("render_spans") == 3 and ix.stat("render_ms") > 0
    # add + rebuild, save / load: the new ids are found
    ix.add(5, b"yellow")
    ix.build()
    store[5] = b"yellow"
    check(ix, store, [5, 30, 10, 20, 6], [b"lo", b"ll"])
    path = str(tmp_path / "idx")
    ix.save(path)
    other = capi.GpuStringIndex()
    other.load(path)
    check(other, store, [5, 30, 10, 20, 6], [b"lo", b"ll"])


def test_ascending_and_shuffled_ids_agree():
    rng = random.Random(21)
    docs = [bytes(rng.choice(b"xyz") for _ in range(rng.randrange(40))) for _ in range(700)]
    asc, store_a = make_index(docs)
    perm = rng.sample(range(700), 700)
    shuf, store_s = make_index(docs, ids=[7 + 3 * p for p in perm])
    page = [7 + 3 * rng.randrange(-5, 720) for _ in range(900)]
    check(asc, store_a, page, [b"xy", b"zz"])
    check(shuf, store_s, page, [b"xy", b"zz"])


# ---- 9. resident text ------------------------------------------------------------------------------------------------------
def test_resident_build_renders_like_host_build():
    import torch
    rng = random.Random(31)
    docs = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(90))) for _ in range(400)]
    host, store = make_index(docs)
    ids = np.array(sorted(store), dtype=np.int64)
    ds = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    text = torch.from_numpy(np.frombuffer(b"".join(docs), dtype=np.uint8).copy()).cuda()
    d_ds, d_ids = torch.from_numpy(ds).cuda(), torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    res = capi.GpuStringIndex()
    res.build_resident(text.data_ptr(), d_ds.data_ptr(), d_ids.data_ptr(), len(docs))
    page = [int(rng.choice(ids)) + rng.choice([0, 0, 0, 1]) for _ in range(300)]
    a = host.render_rows(page, [b"ab", b"cc"], b"<", b">", raw=True)
    b = check(res, store, page, [b"ab", b"cc"], b"<", b">")
    assert a["text_blob"] == b["text_blob"] and a["begin"].tolist() == b["begin"].tolist()


# ---- 10. shards ------------------------------------------------------------------------------------------------------------
def test_three_shards_equal_the_single_index():
    rng = random.Random(41)
    docs = [bytes(rng.choice(b"abc") for _ in range(rng.randrange(90))) for _ in range(900)]
    one, store = make_index(docs)
    sh = capi.GpuShards([0, 0, 0])
    sh.set_option("use_all_devices", 1)
    ids = np.array(sorted(store), dtype=np.int64)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    sh.add_bulk(ids, np.frombuffer(b"".join(docs), dtype=np.uint8), ds)
    sh.build()
    assert sh.count == 3
    page = [int(rng.choice(ids)) + rng.choice([0, 0, 0, 0, 1]) for _ in range(500)]
    a = one.render_rows(page, [b"ab", b"bca", b"cc"], b"[", b"]", raw=True)
    b = check(sh, store, page, [b"ab", b"bca", b"cc"], b"[", b"]")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert 0 < b["missing"] < len(page)


# ---- 11. concurrency -------------------------------------------------------------------------------------------------------
def test_eight_threads_on_one_handle():
    rng = random.Random(51)
    docs = [bytes(rng.choice(b"ab") for _ in range(rng.randrange(120))) for _ in range(600)]
    ix, store = make_index(docs)
    have = sorted(store)
    jobs = [([rng.choice(have) for _ in range(150)], [b"ab" * (1 + t % 3), b"bb", bytes([97 + t % 2])]) for t in range(8)]
    errors = []

    def work(page, kws):
        try:
            for _ in range(3):
                check(ix, store, page, kws)
        except BaseException as e:   # noqa: BLE001 (reported below, on the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
