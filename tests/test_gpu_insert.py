"""cdb_insert_objects (capi.insert_objects): objects join every field given, all or none.

The database is a Python model — per string field the (id, document) pairs in insertion order, per column a column_referee.RefColumn,
and tests/insert_referee.py for what a call must answer.  After every successful call each string field must equal a FRESH build over
the model's documents (layout, suffix array, query rows), each column's four arrays must equal the referee's, and cdb_rowset_all over
the fields must give the union of the model's ids.  After every refusal every array is byte for byte what it was.  The inputs are tiny:
string fields of at most 64 documents, columns of at most about a thousand rows."""
import numpy as np
import pytest
import torch

from coffeedb_amd import capi
from tests import column_referee as CR
from tests import insert_referee as R

pytestmark = pytest.mark.gpu

E_INVALID, E_DEVICE = 1, 2
KEYWORDS = [b"ab", b"a", b"dcb", b"\xc3\xa9", b"bcda"]


def pack(docs):
    blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    return blob, ds


def make_docs(rng, n, hi=False, empty_every=0):
    alphabet = np.frombuffer(b"ab\xc3\xa9" if hi else b"abcd", dtype=np.uint8)
    docs = [alphabet[rng.integers(0, 4, int(l))].tobytes() for l in rng.integers(3, 30, n)]
    if empty_every:
        docs = [b"" if j % empty_every == 1 else d for j, d in enumerate(docs)]
    return docs


class Field:
    """a handle and its model.  kind: "s" string index, or a column kind 0 / 1 / 2"""

    def __init__(self, kind, ids=(), payload=(), build=True):
        self.kind = kind
        ids = np.asarray(ids, dtype=np.int64)
        if kind == "s":
            self.h = capi.GpuStringIndex(device=0)
            self.ids, self.docs = ids.copy(), list(payload)
            if build:
                self.h.add_bulk(ids, *pack(self.docs))
                self.h.build()
        else:
            self.h = capi.GpuColumn(kind, device=0)
            self.ref = CR.RefColumn(kind)
            if build:
                if len(ids):
                    self.h.add_bulk(ids, payload)
                    self.ref.build(ids, payload)
                self.h.build()

    def close(self):
        self.h.close()

    def held(self):
        return self.ids if self.kind == "s" else self.ref.ids

    def payload(self, payload):
        return pack(payload) if self.kind == "s" else payload

    def model_append(self, ids, payload):
        if not len(ids):
            return
        if self.kind == "s":
            self.ids, self.docs = np.concatenate([self.ids, ids]), self.docs + list(payload)
        else:
            self.ref.append(ids, payload)

    def snapshot(self):
        if self.kind == "s":
            g = self.h
            return (g.size, g.bits, g.mask, g.sa_width, g.sa().tobytes() if g.sa_width else b"")
        return tuple(a.tobytes() for a in self.h.arrays())

    def appends(self):
        return self.h.stat("appends")

    def check(self):
        if self.kind == "s":
            g = self.h
            f = capi.GpuStringIndex(device=0)
            try:
                f.add_bulk(self.ids, *pack(self.docs))
                f.build()
                assert (g.size, g.bits, g.mask, g.sa_width) == (f.size, f.bits, f.mask, f.sa_width)
                assert np.array_equal(g.sa(), f.sa())
                for kw in KEYWORDS:
                    assert g.query(kw) == f.query(kw), kw
            finally:
                f.close()
        else:
            c, ref = self.h, self.ref
            assert c.stat("rows") == len(ref.ids) and c.stat("staged_rows") == 0
            for name, got, want in zip(("keys_v", "ids_v", "id_sorted", "vpos"), c.arrays(), ref.arrays()):
                assert got.dtype == want.dtype and np.array_equal(got, want), name
            if ref.kind == 0 and len(ref.ids):
                assert len(c.query_ids("false")) == ref.n_false


def check_all(fields):
    for f in fields:
        f.check()
    with capi.rowset_all([f.h for f in fields]) as rs:
        want = np.unique(np.concatenate([f.held() for f in fields]))
        assert np.array_equal(rs.rows()[0], want)


def insert(fields, ids, parts):
    """parts: per field (rows or None, payload in the model's form)"""
    return capi.insert_objects(ids, [(f.h, rows, f.payload(p)) for f, (rows, p) in zip(fields, parts)])


def insert_and_check(fields, ids, parts):
    ids = np.asarray(ids, dtype=np.int64)
    before = [f.appends() for f in fields]
    inserted, res = insert(fields, ids, parts)
    assert inserted == len(ids)
    for f, (rows, p), r, b in zip(fields, parts, res, before):
        n = len(ids) if rows is None else len(rows)
        assert r == {"appended": n, "status": 0, "committed": int(n > 0)}
        f.model_append(ids if rows is None else ids[np.asarray(rows, dtype=np.int64)], p)
        assert f.appends() == b + int(n > 0)
    check_all(fields)
    return res


def refused(fields, ids, parts, match, code=E_INVALID, lead_inserts=0):
    """two refused calls: nothing moves, and the allocator's in-use level is equal from one refused call to the next"""
    before = [f.snapshot() for f in fields]
    appends = [f.appends() for f in fields]
    in_use = None
    for _ in range(2):   # (the first call warms the lead's kept work spaces and an index's id table)
        with pytest.raises(capi.InsertObjectsError, match=match) as e:
            insert(fields, ids, parts)
        assert e.value.code == code
        assert all((r["appended"], r["committed"]) == (0, 0) for r in e.value.fields)
        assert [f.snapshot() for f in fields] == before
        now = capi.memory_stats()[0]
        assert in_use is None or now == in_use
        in_use = now
    assert [f.appends() for f in fields] == appends
    assert capi.insert_stat(fields[0].h, "inserts") == lead_inserts
    return e.value


def close_all(fields):
    for f in fields:
        f.close()


# ---- field shapes in one call --------------------------------------------------------------------------------------------------
OLD = 1000 + 3 * np.arange(40, dtype=np.int64)
NOLD = len(OLD)


def shapes_db(rng):
    """S, T string fields (T's ids inserted shuffled: its id table is a sorted copy), int64 / double / bool columns with shuffled ids;
    U a never-built index and n a never-built column"""
    t_ids = rng.permutation(OLD)[:30]
    c_ids = rng.permutation(OLD)[:35]
    lv = rng.integers(-20, 20, 35)
    return [Field("s", OLD, make_docs(rng, NOLD)), Field("s", t_ids, make_docs(rng, 30)), Field(1, c_ids, CR.values_of(1, lv)),
            Field(2, c_ids, CR.values_of(2, lv)), Field(0, c_ids, CR.values_of(0, lv)), Field("s", build=False), Field(1, build=False)]


def test_field_shapes_in_one_call():
    rng = np.random.default_rng(20261021)
    fields = shapes_db(rng)
    try:
        # ids descending and interleaved with the old ones (the id merge that is no concatenation); empty documents among them
        ids = (OLD[::4] + 1)[::-1].copy()
        n = len(ids)
        sub = lambda k: np.flatnonzero(np.arange(n) % k != 0).astype(np.uint64)   # proper subsets, strictly ascending
        lv = rng.integers(-20, 20, n)
        parts = [(None, make_docs(rng, n, empty_every=4)), (sub(2), make_docs(rng, len(sub(2)), empty_every=3)),
                 (sub(3), CR.values_of(1, lv[: len(sub(3))])), (None, CR.values_of(2, lv)), (np.empty(0, dtype=np.uint64), CR.values_of(0, [])),
                 (sub(5), make_docs(rng, len(sub(5)))), (sub(2), CR.values_of(1, lv[: len(sub(2))]))]
        assert isinstance(R.insert({k: dict.fromkeys(f.held().tolist()) for k, f in enumerate(fields)}, ids,
                                   [(k, r, list(range(n if r is None else len(r)))) for k, (r, _) in enumerate(parts)]), dict)
        insert_and_check(fields, ids, parts)
        lead = fields[0].h
        assert [capi.insert_stat(lead, s) for s in ("inserts", "insert_fields", "insert_objects")] == [1, 7, n]
        assert capi.insert_stat(lead, "insert_ms") > 0
        # the paths every field took: merges into built fields, the build of the batch in the two that held nothing
        assert [f.h.stat("append_merges") for f in fields] == [1, 1, 1, 1, 0, 0, 0]
        assert [f.h.stat("append_rebuilds") for f in fields] == [0, 0, 0, 0, 0, 1, 1]
        assert fields[2].h.stat("append_id_concat") == 0 and fields[2].h.stat("append_rows") == len(sub(3))
        assert fields[0].h.stat("append_docs") == n
        # every id above every old one: the columns' id order is a concatenation; the bool column takes part this time
        ids2 = 5000 + np.arange(14, dtype=np.int64)
        lv = rng.integers(-20, 20, 14)
        parts2 = [(None, make_docs(rng, 14))] + [(np.empty(0, dtype=np.uint64), [])] + [(None, CR.values_of(k, lv)) for k in (1, 2, 0)] + \
                 [(np.empty(0, dtype=np.uint64), []), (np.arange(1, 14, dtype=np.uint64), CR.values_of(1, lv[1:]))]
        insert_and_check(fields, ids2, parts2)
        assert [fields[k].h.stat("append_id_concat") for k in (2, 3, 4, 6)] == [1, 1, 1, 1]
        assert capi.insert_stat(lead, "inserts") == 2
        # an empty batch is valid, changes nothing and counts no call
        assert insert(fields[:2], np.empty(0, dtype=np.int64), [(None, []), (None, [])]) == (0, [{"appended": 0, "status": 0, "committed": 0}] * 2)
        assert capi.insert_stat(lead, "inserts") == 2 and fields[0].appends() == 2
    finally:
        close_all(fields)


def test_a_column_leads_and_the_profile_holds_the_id_check():
    rng = np.random.default_rng(5)
    fields = [Field(1, OLD, CR.values_of(1, rng.integers(-9, 9, NOLD))), Field("s", OLD[:30], make_docs(rng, 30))]
    try:
        fields[0].h.set_option("profile", 1)
        ids = np.array([7, -7, 3], dtype=np.int64)
        insert_and_check(fields, ids, [(None, CR.values_of(1, [1, 2, 3])), (np.array([1], dtype=np.uint64), [b"abab"])])
        prof = fields[0].h.profile()
        assert {"ins_keys", "ins_count", "ins_fresh"} <= set(prof) and "ins_twice" not in prof
        assert capi.insert_stat(fields[0].h, "inserts") == 1 and capi.insert_stat(fields[1].h, "inserts") == 0
    finally:
        close_all(fields)


# ---- the id check at its edges (tests/insert_referee.py: fresh_cases) ----------------------------------------------------------
CASES = R.fresh_cases()


def case_fields(lists, rng):
    """field k holds lists[k]: even k an int64 column, odd k a string index whose documents went in in shuffled id order (its id table
    is a sorted copy); an empty list is a field that was never built"""
    out = []
    for k, l in enumerate(lists):
        ids = rng.permutation(l)
        if k % 2:
            out.append(Field("s", ids, make_docs(rng, len(ids)), build=len(ids) > 0))
        else:
            out.append(Field(1, ids, CR.values_of(1, rng.integers(-5, 5, len(ids))), build=len(ids) > 0))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_id_check_case(name):
    lists, ids, want, _ = CASES[name]
    rng = np.random.default_rng(len(name))
    fields = case_fields(lists, rng)
    try:
        n = len(ids)
        # a column is offered every object, a string field the first 40 at most (the tiny-input rule); the check reads every id all the same
        few = np.arange(min(n, 40), dtype=np.uint64)
        parts = [(few, [b"ab"[: 1 + j % 2] for j in range(len(few))]) if f.kind == "s" else (None, CR.values_of(1, np.arange(n) % 7)) for f in fields]
        if want is None:
            insert_and_check(fields, ids, parts)
        else:
            text = (f"^cdb_insert_objects: object id {want.id} twice in the batch$" if want.kind == "twice" else
                    f"^cdb_insert_objects: object id {want.id} is already held by field {want.field}$")
            refused(fields, ids, parts, text)
    finally:
        close_all(fields)


def test_an_offender_in_a_field_without_rows():
    rng = np.random.default_rng(9)
    fields = [Field("s", OLD[:20], make_docs(rng, 20)), Field(2, [-4, 90, 17], CR.values_of(2, [1, 2, 3]))]
    try:
        ids = np.array([5, 90, 6], dtype=np.int64)
        parts = [(None, [b"a", b"b", b"c"]), (np.empty(0, dtype=np.uint64), [])]
        refused(fields, ids, parts, "^cdb_insert_objects: object id 90 is already held by field 1$")
        insert_and_check(fields, np.array([5, 91, 6], dtype=np.int64), parts)
    finally:
        close_all(fields)


# ---- validation before any device work -----------------------------------------------------------------------------------------
def test_refusals_of_the_validation():
    rng = np.random.default_rng(11)
    fields = [Field("s", OLD[:20], make_docs(rng, 20)), Field(2, OLD[:10], CR.values_of(2, np.arange(10))), Field(1, build=False)]
    try:
        ids = np.array([1, 2, 3], dtype=np.int64)
        docs = [b"a", b"b", b"c"]
        u = lambda *r: np.array(r, dtype=np.uint64)
        refused(fields[:2], ids, [(u(0, 1), docs[:2]), (u(1), [0.5])], "^cdb_insert_objects: object 2 holds no field$")
        refused(fields[:2], ids, [(None, docs), (u(1, 1), [0.5, 1.5])], "^cdb_insert_objects: field 1: rows must ascend strictly")
        refused(fields[:2], ids, [(None, docs), (u(2, 1), [0.5, 1.5])], "^cdb_insert_objects: field 1: rows must ascend strictly")
        refused(fields[:2], ids, [(None, docs), (u(3), [0.5])], "^cdb_insert_objects: field 1: rows must ascend strictly")
        refused(fields[:2], ids, [(None, docs), (u(0, 2), [0.5, float("nan")])], r"^cdb_column_append: NaN is not a valid value \(row 1\)$")
        with pytest.raises(capi.InsertObjectsError) as e:   # the same handle twice: the code alone
            insert([fields[0], fields[1], fields[0]], ids, [(None, docs), (None, [1.0, 2.0, 3.0]), (None, docs)])
        assert e.value.code == E_INVALID
        fields[2].h.add_bulk([5], [1])   # rows staged since the last build
        refused(fields, ids, [(None, docs), (u(), []), (u(0), [4])], "^append: rows were added since the last build$")
        fields[0].h.add(5, b"pending")
        refused(fields[:2], ids, [(None, docs), (u(), [])], "^append: documents were added since the last build$")
    finally:
        close_all(fields)


def test_fields_on_two_gpus_are_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    a = Field(1, [1, 2], [3, 4])
    other = capi.GpuColumn(1, device=1)
    try:
        other.build()
        with pytest.raises(capi.InsertObjectsError, match="^cdb_insert_objects: all fields must live on one GPU$") as e:
            capi.insert_objects([9], [(a.h, None, [1]), (other, None, [1])])
        assert e.value.code == E_INVALID
    finally:
        a.close()
        other.close()


# ---- all or none ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", [0, 1, 2])
@pytest.mark.parametrize("victim", ["index", "column"])
def test_a_failed_prepare_changes_nothing(victim, position):
    rng = np.random.default_rng(position)
    lv = rng.integers(-9, 9, NOLD)
    v = Field("s", OLD[:30], make_docs(rng, 30)) if victim == "index" else Field(2, OLD, CR.values_of(2, lv))
    others = [Field("s", OLD, make_docs(rng, NOLD)), Field(1, rng.permutation(OLD), CR.values_of(1, lv))]
    fields = others[:position] + [v] + others[position:]
    try:
        ids = np.array([2000, 1001, -5, 2500], dtype=np.int64)   # (every field gets rows: every field has a change to prepare)
        parts = [(None, make_docs(rng, 4)) if f.kind == "s" else (None, CR.values_of(f.kind, [4, -4, 0, 9])) for f in fields]
        v.h.set_option("debug_fail_append_prepare", 1)
        e = refused(fields, ids, parts, r"^field %d: debug: append prepare failure requested \(test hook\)$" % position, code=E_DEVICE)
        assert [r["status"] for r in e.fields] == [E_DEVICE if k == position else 0 for k in range(3)]
        v.h.set_option("debug_fail_append_prepare", 0)
        insert_and_check(fields, ids, parts)
        assert capi.insert_stat(fields[0].h, "inserts") == 1
    finally:
        close_all(fields)


def test_a_failed_prepare_of_the_build_of_the_batch():
    """the field that held nothing fails behind its sort: the built fields in front of it drop what they prepared"""
    rng = np.random.default_rng(4)
    fields = [Field("s", OLD[:30], make_docs(rng, 30)), Field(1, OLD, CR.values_of(1, rng.integers(-9, 9, NOLD))), Field(1, build=False)]
    try:
        ids = np.array([7, 8], dtype=np.int64)
        parts = [(None, [b"ab", b"cd"]), (None, CR.values_of(1, [1, 2])), (None, CR.values_of(1, [3, 4]))]
        fields[2].h.set_option("debug_fail_append_prepare", 1)
        refused(fields, ids, parts, "^field 2: debug: append prepare failure requested", code=E_DEVICE)
        fields[2].h.set_option("debug_fail_append_prepare", 0)
        insert_and_check(fields, ids, parts)
    finally:
        close_all(fields)


def test_the_step_behind_the_commit():
    """a reference-order field (reference_compat = 1, bytes >= 0x80) builds its array inside the commit: when that fails the field is
    never built with committed = 1, and the others commit all the same"""
    rng = np.random.default_rng(6)
    fields = [Field("s", OLD[:30], make_docs(rng, 30)), Field("s", OLD[:40], make_docs(rng, 40, hi=True)),
              Field(1, OLD, CR.values_of(1, rng.integers(-9, 9, NOLD)))]
    try:
        ids = np.array([7, 8, 9], dtype=np.int64)
        parts = [(None, make_docs(rng, 3)), (None, make_docs(rng, 3, hi=True)), (None, CR.values_of(1, [1, 2, 3]))]
        fields[1].h.set_option("debug_fail_build", 1)
        with pytest.raises(capi.InsertObjectsError, match="^field 1: debug: build failure requested") as e:
            insert(fields, ids, parts)
        res = e.value.fields
        assert e.value.code == E_INVALID and [r["status"] for r in res] == [0, E_INVALID, 0]
        assert [r["committed"] for r in res] == [1, 1, 1] and [r["appended"] for r in res] == [3, 0, 3]
        assert capi.insert_stat(fields[0].h, "inserts") == 1
        assert fields[1].h.sa_width == 0 and fields[1].h.query(b"ab") == []   # never built
        for k in (0, 2):
            fields[k].model_append(ids, parts[k][1])
            fields[k].check()
    finally:
        close_all(fields)


# ---- one call equals the per-field calls, and the per-field calls are what they were ------------------------------------------------
def test_equals_the_per_field_calls():
    ids = np.array([2000, 1001, -5, 2500, 1004], dtype=np.int64)
    rows = np.array([0, 2, 3], dtype=np.uint64)
    dbs = []
    try:
        for _ in range(2):
            rng = np.random.default_rng(8)
            every = shapes_db(rng)
            close_all(every[5:])
            dbs.append(every[:5])
        rng = np.random.default_rng(80)
        docs, lv = make_docs(rng, 5), rng.integers(-9, 9, 5)
        parts = [(None, docs), (rows, docs[:3]), (None, CR.values_of(1, lv)), (rows, CR.values_of(2, lv[:3])), (None, CR.values_of(0, lv))]
        insert(dbs[0], ids, parts)
        for f, (r, p) in zip(dbs[1], parts):
            fid = ids if r is None else ids[r.astype(np.int64)]
            assert (f.h.append(fid, *pack(p)) if f.kind == "s" else f.h.append(fid, p)) == len(fid)
        assert [f.snapshot() for f in dbs[0]] == [f.snapshot() for f in dbs[1]]
        for a, b in zip(dbs[0], dbs[1]):
            names = ("appends", "append_merges", "append_rebuilds", "append_docs", "append_bytes", "append_keys_kept") if a.kind == "s" else \
                    ("appends", "append_merges", "append_rebuilds", "append_rows", "append_id_concat", "rows", "id_sort_skipped")
            assert [a.h.stat(s) for s in names] == [b.h.stat(s) for s in names]
    finally:
        for d in dbs:
            close_all(d)


def test_column_append_alone_is_what_it_was():
    rng = np.random.default_rng(12)
    for kind in (0, 1, 2):
        f = Field(kind, build=False)
        try:
            c, lv = f.h, rng.integers(-9, 9, 300)
            ids = rng.permutation(300).astype(np.int64) * 5
            assert c.append(ids[:100], CR.values_of(kind, lv[:100])) == f.ref.append(ids[:100], CR.values_of(kind, lv[:100])) == 100
            f.check()   # a column without rows: the build of the batch
            assert [c.stat(s) for s in ("appends", "append_merges", "append_rebuilds", "append_rows", "id_sort_skipped")] == [1, 0, 1, 100, 0]
            assert c.stat("build_ms") > 0
            assert c.append(ids[100:200], CR.values_of(kind, lv[100:200])) == f.ref.append(ids[100:200], CR.values_of(kind, lv[100:200]))
            f.check()   # the merge
            assert [c.stat(s) for s in ("appends", "append_merges", "append_rebuilds", "append_rows", "append_id_concat")] == [2, 1, 1, 100, 0]
            c.set_option("debug_maintain_path", 2)   # the build over old rows and batch
            assert c.append(ids[200:], CR.values_of(kind, lv[200:])) == f.ref.append(ids[200:], CR.values_of(kind, lv[200:]))
            f.check()
            assert [c.stat(s) for s in ("appends", "append_merges", "append_rebuilds", "append_rows")] == [3, 1, 2, 100]
            c.set_option("debug_maintain_path", 0)
            before = f.snapshot()
            with pytest.raises(RuntimeError, match=f"^cdb_column_append: duplicate object id {int(ids[7])} in one column$"):
                c.append([int(ids[7])], CR.values_of(kind, [1]))
            assert f.snapshot() == before and c.stat("appends") == 3
            assert c.append([10**6], CR.values_of(kind, [1])) == f.ref.append([10**6], CR.values_of(kind, [1])) == 1
            f.check()   # every new id above every old one
            assert c.stat("append_id_concat") == 1
            c.set_option("debug_fail_append_prepare", 1)
            before = f.snapshot()
            with pytest.raises(RuntimeError, match="^debug: append prepare failure requested"):
                c.append([10**6 + 1], CR.values_of(kind, [1]))
            assert f.snapshot() == before and c.stat("appends") == 4
        finally:
            f.close()


def test_index_append_alone_is_what_it_was():
    rng = np.random.default_rng(13)
    f = Field("s", OLD[:30], make_docs(rng, 30))
    try:
        g, docs = f.h, make_docs(rng, 8, empty_every=3)
        ids = np.arange(8, dtype=np.int64)
        assert g.append(ids, *pack(docs)) == 8
        f.model_append(ids, docs)
        f.check()
        assert [g.stat(s) for s in ("appends", "append_merges", "append_rebuilds", "append_docs")] == [1, 1, 0, 8]
        g.set_option("debug_fail_append_prepare", 1)
        before = f.snapshot()
        with pytest.raises(RuntimeError, match="^debug: append prepare failure requested"):
            g.append(ids + 100, *pack(docs))
        assert f.snapshot() == before and g.stat("appends") == 1
        g.set_option("debug_fail_append_prepare", 0)
        assert g.append(ids + 100, *pack(docs)) == 8
        f.model_append(ids + 100, docs)
        f.check()
    finally:
        f.close()
