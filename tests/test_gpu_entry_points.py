"""The host halves of the query-side entry points at their own edges (keyword_list.h, host_io.h, capi_query.hip): a keyword list
that is a slice of a larger blob, answers without rows, every refusal with its exact text, and the one resolver behind both ANDs.
Eight short documents (the reference README's three plus a few), one int64 column over the same rows, the sharded index as two
shards co-resident on device 0.  Every entry point is called through ctypes with the test's own blob and offsets: the Python
wrappers pack theirs at base 0.  The expected rows come from tests/ref_model.py; offsets, spans and rendered strings from a few
lines of Python over the documents."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests.ref_model import RefModel

pytestmark = pytest.mark.gpu

DOCS = [b"3010103", b"301022", b"01011010", b"abcabcabc", b"aaaaaa", b"banana 010", b"coffee 0101 abc", b"tea"]
IDS = [100 + d for d in range(len(DOCS))]
VALUES = [1, 2, 3, 4, 5, 6, 7, 8]           # the int64 column, row for row
KW1, KW2 = [b"010", b"abc"], [b"0", b"a"]   # two string keys; every keyword occurs somewhere
HOST_ROWS = [(100, 0), (101, 0), (102, 0), (105, 0), (106, 0), (107, 0)]
RANGE = b"[2,6]"                            # ids 101 .. 105
ABSENT = [b"zzz"]
PAGE = [107, 100, 999, 106, 102]            # rows to render: caller's order, one id the index does not hold
LEFT, RIGHT = b"<b>", b"</b>"
FRONT, BACK = b"\xffJUNK!!", b"??tail\x00"   # seven bytes in front of a sliced list, some behind
INVALID = 1                                 # CDB_E_INVALID
BIG = 1 << 62


# ---- what the answers must be ------------------------------------------------------------------------------------------------------
def _union(model, kws):
    acc = {}
    for kw in kws:
        for i, c in model.query(kw):
            acc[i] = acc.get(i, 0) + c
    return sorted(acc.items())


def _ranked(rows, lo, hi, limit):
    keep = sorted((r for r in rows if lo <= r[1] < hi), key=lambda r: (-r[1], r[0]))
    return keep[:limit] if limit else keep


def _intersect(lists):
    acc = dict(lists[0])
    for rows in lists[1:]:
        d = dict(rows)
        acc = {i: c + d[i] for i, c in acc.items() if i in d}
    return sorted(acc.items())


def _occurrences(doc, kw):
    return [p for p in range(len(doc) - len(kw) + 1) if doc[p:p + len(kw)] == kw]


def _spans(doc, kws):
    """the highlight spans of database.cpp:58-77, ends inclusive: occurrences that overlap merge, occurrences that only touch do not"""
    occ = sorted((p, p + len(kw)) for kw in kws for p in _occurrences(doc, kw))
    out = []
    for a, b in occ:
        if out and a < out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, b - 1) for a, b in out]


def _rendered(doc, kws):
    text, at = b"", 0
    for a, e in _spans(doc, kws):
        text += doc[at:a] + LEFT + doc[a:e + 1] + RIGHT
        at = e + 1
    return text + doc[at:]


# ---- keyword lists as the C ABI takes them -----------------------------------------------------------------------------------------
class Kw:
    """blob + offsets of a keyword list: at base 0, or as a slice of a larger blob (offsets[0] == 7, junk on both sides)"""

    def __init__(self, kws, sliced=False, blob=True, offsets=True, offs=None):
        front = FRONT if sliced else b""
        self.blob = np.frombuffer(front + b"".join(kws) + (BACK if sliced else b"") + b"\x00", dtype=np.uint8).copy()
        self.offs = np.array(np.cumsum([len(front)] + [len(k) for k in kws]) if offs is None else offs, dtype=np.uint64)
        self.n = len(kws)
        self.p = self.blob.ctypes.data if blob else None
        self.o = self.offs.ctypes.data if offsets else None


def _rows(lib, ids, cnt, n):
    assert bool(ids) and bool(cnt), "a result without rows still has arrays"
    out = [(int(ids[i]), int(cnt[i])) for i in range(n.value)]
    lib.cdb_free(ids)
    lib.cdb_free(cnt)
    return out


def _rows_out():
    return C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)


def _key_array(keys):
    """[(handle or None, Kw or [(id, count), ...] or None)]: a string key, host rows, or a row list that is missing"""
    from coffeedb_amd import capi
    arr, keep = (capi.CdbKeyQuery * len(keys))(), []
    for k, (h, data) in enumerate(keys):
        if h is not None:
            arr[k].index, arr[k].blob, arr[k].offsets, arr[k].nkw = h, data.p, data.o, data.n
        elif data is None:
            arr[k].nrows = 2
        else:
            ri, rc = np.array([r[0] for r in data], dtype=np.int64), np.array([r[1] for r in data], dtype=np.int64)
            keep += [ri, rc]
            arr[k].ids, arr[k].counts, arr[k].nrows = ri.ctypes.data, rc.ctypes.data, len(data)
    return arr, keep


class Calls:
    """every entry point as f(...) -> (status, answer): the answer normalised to Python values, its arrays checked non-null and freed"""

    def __init__(self, db):
        from coffeedb_amd import capi
        self.capi, self.lib, self.db = capi, capi.load_library(), db

    def _batch(self, fn, h, kw, with_hits):
        r, hits = self.capi.CdbResult(), self.capi.CdbHits()
        rc = fn(h, kw.p, kw.o, kw.n, C.byref(r), C.byref(hits)) if with_hits else fn(h, kw.p, kw.o, kw.n, C.byref(r))
        if rc:
            assert not r.row_ptr and not r.ids and not r.counts and not hits.hit_ptr and not hits.offsets, "a refused call left arrays"
            return rc, None
        assert r.npat == kw.n and bool(r.row_ptr) and bool(r.ids) and bool(r.counts)
        assert r.row_ptr[0] == 0 and r.row_ptr[kw.n] == r.nrows
        if with_hits:
            assert bool(hits.hit_ptr) and bool(hits.offsets) and hits.hit_ptr[0] == 0 and hits.hit_ptr[r.nrows] == r.nhits
        out = []
        for j in range(kw.n):
            rows = [(int(r.ids[i]), int(r.counts[i])) for i in range(r.row_ptr[j], r.row_ptr[j + 1])]
            if with_hits:
                rows = [row + ([int(hits.offsets[k]) for k in range(hits.hit_ptr[i], hits.hit_ptr[i + 1])],)
                        for row, i in zip(rows, range(r.row_ptr[j], r.row_ptr[j + 1]))]
            out.append(rows)
        self.lib.cdb_result_free(C.byref(r))
        self.lib.cdb_hits_free(C.byref(hits))
        assert not r.row_ptr and not hits.hit_ptr
        return rc, out

    def batch(self, kw):
        return self._batch(self.lib.cdb_query_batch, self.db.one._h, kw, False)

    def batch_offsets(self, kw):
        return self._batch(self.lib.cdb_query_batch_offsets, self.db.one._h, kw, True)

    def shards_batch(self, kw, device_merge=0):
        self.db.sh.set_option("device_merge", device_merge)
        try:
            return self._batch(self.lib.cdb_shards_query_batch, self.db.sh._h, kw, False)
        finally:
            self.db.sh.set_option("device_merge", 0)

    def shards_batch_device(self, kw):
        return self.shards_batch(kw, 1)

    def q_or(self, kw):
        ids, cnt, n = _rows_out()
        rc = self.lib.cdb_query_or(self.db.one._h, kw.p, kw.o, kw.n, C.byref(ids), C.byref(cnt), C.byref(n))
        return rc, None if rc else _rows(self.lib, ids, cnt, n)

    def ranked(self, kw, lo=1, hi=BIG, limit=3):
        ids, cnt, n = _rows_out()
        rc = self.lib.cdb_query_ranked(self.db.one._h, kw.p, kw.o, kw.n, lo, hi, limit, C.byref(ids), C.byref(cnt), C.byref(n))
        return rc, None if rc else _rows(self.lib, ids, cnt, n)

    def spans(self, kw):
        r = self.capi.CdbSpans()
        rc = self.lib.cdb_query_spans(self.db.one._h, kw.p, kw.o, kw.n, C.byref(r))
        if rc:
            assert not r.ids and not r.span_ptr and not r.begin and not r.end
            return rc, None
        assert bool(r.ids) and bool(r.span_ptr) and bool(r.begin) and bool(r.end) and r.span_ptr[0] == 0 and r.span_ptr[r.ndocs] == r.nspans
        out = [(int(r.ids[d]), [(int(r.begin[k]), int(r.end[k])) for k in range(r.span_ptr[d], r.span_ptr[d + 1])]) for d in range(r.ndocs)]
        self.lib.cdb_spans_free(C.byref(r))
        return rc, out

    def _and(self, fn, keys, ranked=0, lo=1, hi=BIG, limit=0, cols=None):
        arr, keep = _key_array(keys)
        ids, cnt, n = _rows_out()
        tail = (ranked, lo, hi, limit, C.byref(ids), C.byref(cnt), C.byref(n))
        rc = fn(arr, len(keys), *tail) if cols is None else fn(arr, len(keys), cols[0], cols[1], *tail)
        return rc, None if rc else _rows(self.lib, ids, cnt, n)

    def _string_keys(self, h, kw):
        return [(h, kw), (h, Kw(KW2, sliced=True)), (None, HOST_ROWS)]

    def q_and(self, kw, **o):
        return self._and(self.lib.cdb_query_and, self._string_keys(self.db.one._h, kw), **o)

    def shards_and(self, kw, **o):
        return self._and(self.lib.cdb_shards_query_and, self._string_keys(self.db.sh._h, kw), **o)

    def _column_key(self, with_column):
        carr = (self.capi.CdbColumnKey * 1)()
        self._range = np.frombuffer(FRONT + RANGE + BACK, dtype=np.uint8).copy()
        self._range_offs = np.array([len(FRONT), len(FRONT) + len(RANGE)], dtype=np.uint64)
        carr[0].column, carr[0].blob, carr[0].offsets, carr[0].nranges = self.db.col._h, self._range.ctypes.data, self._range_offs.ctypes.data, 1
        return (carr, 1) if with_column else (None, 0)

    def and_columns(self, kw, with_column=True, **o):
        return self._and(self.lib.cdb_query_and_columns, self._string_keys(self.db.one._h, kw), cols=self._column_key(with_column), **o)

    def filter(self, kw):
        arr, keep = _key_array(self._string_keys(self.db.one._h, kw))
        carr, nc = self._column_key(True)
        h = C.c_void_p()
        rc = self.lib.cdb_filter(arr, 3, carr, nc, 0, 0, 0, C.byref(h))
        if rc:
            assert not h
            return rc, None
        with self.capi.GpuRowSet(h) as rs:
            ids, counts = rs.rows()
            assert len(rs) == len(ids)
            return rc, [(int(i), int(c)) for i, c in zip(ids, counts)]

    def _render(self, fn, h, kw):
        page = np.array(PAGE, dtype=np.int64)
        r = self.capi.CdbRendered()
        rc = fn(h, page.ctypes.data, len(page), kw.p, kw.o, kw.n, LEFT, len(LEFT), RIGHT, len(RIGHT), 3, C.byref(r))
        if rc:
            assert not r.found and not r.text_ptr and not r.text_blob and not r.span_ptr and not r.begin and not r.end
            return rc, None
        n = len(page)
        assert all(bool(p) for p in (r.found, r.text_ptr, r.text_blob, r.span_ptr, r.begin, r.end))
        blob = C.string_at(r.text_blob, int(r.text_bytes))
        out = ([bool(r.found[i]) for i in range(n)], int(r.missing), [blob[r.text_ptr[i]:r.text_ptr[i + 1]] for i in range(n)],
               [[(int(r.begin[k]), int(r.end[k])) for k in range(r.span_ptr[i], r.span_ptr[i + 1])] for i in range(n)])
        self.lib.cdb_rendered_free(C.byref(r))
        return rc, out

    def render(self, kw):
        return self._render(self.lib.cdb_render_rows, self.db.one._h, kw)

    def select(self, kw):
        """the page of the whole-database row set with one string field highlighted by kw: (ids, texts)"""
        f = (self.capi.CdbSelectField * 1)()
        f[0].index, f[0].kw_blob, f[0].kw_offsets, f[0].nkw = self.db.one._h, kw.p, kw.o, kw.n
        r = self.capi.CdbSelected()
        rc = self.lib.cdb_rowset_select(self.db.rs._h, 0, 3, f, 1, LEFT, len(LEFT), RIGHT, len(RIGHT), C.byref(r))
        if rc:
            assert not r.ids and not r.counts and not r.fields
            return rc, None
        g = r.fields[0]
        blob = C.string_at(g.text_blob, int(g.text_ptr[r.nrows]))
        out = ([int(r.ids[i]) for i in range(r.nrows)], [blob[g.text_ptr[i]:g.text_ptr[i + 1]] for i in range(r.nrows)])
        self.lib.cdb_selected_free(C.byref(r))
        return rc, out

    def error_of(self, name):
        if name.startswith("shards"):
            return self.lib.cdb_shards_last_error(self.db.sh._h).decode()
        if name == "select":
            return self.lib.cdb_rowset_last_error(self.db.rs._h).decode()
        return self.lib.cdb_last_error(self.db.one._h).decode()


@pytest.fixture(scope="module")
def db():
    from coffeedb_amd import capi
    blob = np.frombuffer(b"".join(DOCS), dtype=np.uint8)
    ds = np.array(np.cumsum([0] + [len(d) for d in DOCS]), dtype=np.uint64)
    ids = np.array(IDS, dtype=np.int64)
    one = capi.GpuStringIndex(device=0)
    one.add_bulk(ids, blob, ds)
    one.build()
    sh = capi.GpuShards([0, 0])
    sh.set_option("use_all_devices", 1)
    sh.add_bulk(ids, blob, ds)
    sh.build()
    assert sh.count == 2
    col = capi.GpuColumn("int64", device=0)
    col.add_bulk(ids, VALUES)
    col.build()
    rs = capi.debug_rowset_from_rows(ids, np.arange(len(IDS), 0, -1), device=0)   # counts descend: the page is ids 100, 101, 102
    d = SimpleNamespace(one=one, sh=sh, col=col, rs=rs, model=RefModel(IDS, DOCS))
    d.calls = Calls(d)
    yield d
    for h in (rs, col, sh, one):
        h.close()


def _expected(model, name, kws):
    """the answer of entry point `name` for the first string key's keywords kws, stated from the model and the documents"""
    k1, k2 = _union(model, kws), _union(model, KW2)
    in_range = [(i, 0) for i, v in zip(IDS, VALUES) if 2 <= v <= 6]
    doc_of = dict(zip(IDS, DOCS))
    if name in ("batch", "shards_batch", "shards_batch_device"):
        return [model.query(kw) for kw in kws]
    if name == "batch_offsets":
        return [[(i, c, _occurrences(doc_of[i], kw)) for i, c in model.query(kw)] for kw in kws]
    if name == "q_or":
        return k1
    if name == "ranked":
        return _ranked(k1, 1, BIG, 3)
    if name == "spans":
        return [(i, _spans(doc_of[i], kws)) for i, _ in k1]
    if name in ("q_and", "shards_and"):
        return _intersect([k1, k2, HOST_ROWS])
    if name in ("and_columns", "filter"):
        return _intersect([k1, k2, HOST_ROWS, in_range])
    if name == "render":
        found = [i in doc_of for i in PAGE]
        return (found, found.count(False), [_rendered(doc_of[i], kws) if i in doc_of else b"" for i in PAGE],
                [_spans(doc_of[i], kws) if i in doc_of else [] for i in PAGE])
    if name == "select":
        return (IDS[:3], [_rendered(doc_of[i], kws) for i in IDS[:3]])
    raise KeyError(name)


ENTRY_POINTS = ["batch", "batch_offsets", "q_or", "ranked", "spans", "q_and", "and_columns", "filter", "render", "shards_batch",
                "shards_batch_device", "shards_and"]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_a_keyword_list_sliced_out_of_a_larger_blob_answers_as_at_base_zero(db, name):
    f = getattr(db.calls, name)
    sliced = Kw(KW1, sliced=True)
    assert sliced.offs[0] == 7
    rc0, at_zero = f(Kw(KW1))
    rc7, at_seven = f(sliced)
    assert rc0 == 0 and rc7 == 0
    want = _expected(db.model, name, KW1)
    assert at_zero == want
    assert at_seven == want


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_a_keyword_that_occurs_nowhere_gives_no_rows_and_arrays_that_free(db, name):
    rc, got = getattr(db.calls, name)(Kw(ABSENT, sliced=True))   # (the helpers check every array non-null, and free them)
    assert rc == 0
    want = _expected(db.model, name, ABSENT)
    assert got == want
    if name == "render":   # the plain documents, no span
        assert got[2] == [dict(zip(IDS, DOCS)).get(i, b"") for i in PAGE] and not any(got[3])
    else:
        assert got == ([[]] if "batch" in name else [])


@pytest.mark.parametrize("name", ["batch", "batch_offsets", "shards_batch", "shards_batch_device"])
@pytest.mark.parametrize("offsets", [True, False])
def test_a_batch_of_no_patterns_is_an_empty_result(db, name, offsets):
    rc, got = getattr(db.calls, name)(Kw([], sliced=True, offsets=offsets))
    assert rc == 0 and got == []


EMPTY_KW = "Empty keywords are not allowed"
EMPTY_LIST = "The constraint list cannot be empty"


def _bad(what):
    """a first string key that is wrong in one way (the other keys of an AND stay sound)"""
    return {"empty keyword": Kw([b"010", b"", b"abc"], sliced=True), "empty first keyword": Kw([b"", b"abc"]),
            "decreasing offsets": Kw(KW1, offs=[0, 3, 1]),
            "empty list": Kw([], sliced=True), "missing offsets": Kw(KW1, offsets=False), "no bytes": Kw(KW1, blob=False)}[what]


# (entry point, bad input) -> (status, text in the handle's last error; None: refused before anything could carry a text).
# The texts are the parent commit's, recorded by running this table against its library.
ERROR_TABLE = [
    ("batch", "empty keyword", EMPTY_KW), ("batch", "empty first keyword", EMPTY_KW), ("batch", "missing offsets", None),
    ("batch_offsets", "empty keyword", EMPTY_KW), ("batch_offsets", "missing offsets", None),
    ("q_or", "empty keyword", EMPTY_KW), ("q_or", "empty list", EMPTY_LIST), ("q_or", "missing offsets", None),
    ("ranked", "empty keyword", EMPTY_KW), ("ranked", "empty list", EMPTY_LIST), ("ranked", "missing offsets", None),
    ("spans", "missing offsets", None),
    ("q_and", "empty keyword", EMPTY_KW), ("q_and", "empty list", EMPTY_LIST),
    ("q_and", "missing offsets", "cdb_query_and: keyword offsets missing"), ("q_and", "missing rows", "cdb_query_and: row list missing"),
    ("and_columns", "empty keyword", EMPTY_KW), ("and_columns", "empty list", EMPTY_LIST),
    ("and_columns", "missing offsets", "cdb_query_and_columns: keyword offsets missing"),
    ("and_columns", "missing rows", "cdb_query_and_columns: row list missing"),
    ("filter", "empty keyword", EMPTY_KW), ("filter", "empty list", EMPTY_LIST),
    ("filter", "missing offsets", "cdb_query_and_columns: keyword offsets missing"),
    ("filter", "missing rows", "cdb_query_and_columns: row list missing"),
    ("render", "empty keyword", EMPTY_KW), ("render", "missing offsets", None), ("render", "no bytes", "cdb_render_rows: keywords without bytes"),
    ("select", "empty keyword", EMPTY_KW), ("select", "missing offsets", None), ("select", "no bytes", "cdb_rowset_select: keywords without bytes"),
    ("shards_batch", "empty keyword", EMPTY_KW), ("shards_batch", "missing offsets", None),
    ("shards_batch_device", "empty keyword", EMPTY_KW), ("shards_batch_device", "missing offsets", None),
    ("shards_and", "empty keyword", EMPTY_KW), ("shards_and", "empty list", EMPTY_LIST),
    ("shards_and", "missing offsets", "cdb_shards_query_and: keyword offsets missing"),
    ("shards_and", "missing rows", "cdb_shards_query_and: row list missing"),
]


@pytest.mark.parametrize("name,what,text", ERROR_TABLE, ids=[f"{n}-{w.replace(' ', '_')}" for n, w, _ in ERROR_TABLE])
def test_every_refusal_has_its_status_and_text_and_leaves_the_handle_serving(db, name, what, text, monkeypatch):
    calls = db.calls
    f = getattr(calls, name)
    if what == "missing rows":   # the host-row key announces rows and gives none
        monkeypatch.setattr(calls, "_string_keys", lambda h, kw: [(h, kw), (h, Kw(KW2)), (None, None)])
        rc, got = f(Kw(KW1))
        monkeypatch.undo()
    else:
        rc, got = f(_bad(what))
    assert rc == INVALID and got is None
    if text is not None:
        assert calls.error_of(name) == text
    # no lock was left held and no half result behind: the same handles answer a sound call
    rc, got = f(Kw(KW1, sliced=True))
    assert rc == 0 and got == _expected(db.model, name, KW1)


def test_decreasing_offsets_count_as_an_empty_keyword(db):
    for name in ("batch", "q_or", "q_and", "render"):
        rc, got = getattr(db.calls, name)(_bad("decreasing offsets"))
        assert rc == INVALID and got is None and db.calls.error_of(name) == EMPTY_KW


@pytest.mark.parametrize("ranked,lo,hi,limit", [(0, 1, BIG, 0), (1, 1, BIG, 0), (1, 1, BIG, 3), (1, 2, 5, 0), (1, 2, BIG, 2)])
def test_both_ands_resolve_string_and_host_keys_through_one_resolver(db, ranked, lo, hi, limit):
    """cdb_query_and over {string key, string key on the same handle, host rows} = cdb_query_and_columns with the same keys and no
    column key = the model, unranked and ranked, with a limit below the row count"""
    calls, kw = db.calls, Kw(KW1, sliced=True)
    rows = _intersect([_union(db.model, KW1), _union(db.model, KW2), HOST_ROWS])
    assert len(rows) == 5
    want = _ranked(rows, lo, hi, limit) if ranked else rows
    assert 0 < len(want) and (not limit or len(want) == limit < len(rows))
    o = dict(ranked=ranked, lo=lo, hi=hi, limit=limit)
    assert calls.q_and(kw, **o) == (0, want)
    assert calls.and_columns(kw, with_column=False, **o) == (0, want)
    assert calls.shards_and(kw, **o) == (0, want)


def test_spans_drop_empty_keywords_instead_of_refusing_them(db):
    want = _expected(db.model, "spans", KW1)
    assert db.calls.spans(Kw([b"", b"010", b"", b"abc", b""], sliced=True)) == (0, want)
    assert db.calls.spans(Kw([b"", b""], sliced=True)) == (0, [])
    assert db.calls.spans(Kw([], sliced=True)) == (0, [])
