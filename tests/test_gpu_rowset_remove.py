"""cdb_rowset_remove (capi.GpuRowSet.remove): the rows of a set leave every field given, all or none, with the ids staying on the device.

The database is a Python model — per string field the (id, document) pairs in insertion order, per column a column_referee.RefColumn —
over 3 * 4096 + 1 ids (the 4096-slot tiles of stable_tiles.h are crossed, every build takes milliseconds):

    A   every id, inserted ascending           (variant `hi`: bytes >= 0x80 under reference_compat = 1: the rebuild path)
    B   every second id
    C   a third of the ids, inserted in shuffled order: ids do not ascend by document (the id_doc path of rm_mark)
    b / i / d   bool, int64, double columns: ids inserted in shuffled order, every fifth id absent

After every call each string field must equal a FRESH build over the model's survivors (layout, suffix array, query rows), each
column's four arrays must equal the referee's, removed / missing must equal the model's and add up to the set's size."""
import threading

import numpy as np
import pytest
import torch

from coffeedb_amd import capi
from tests import column_referee as CR

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 1
IDS = 1000 + 3 * np.arange(N, dtype=np.int64)
KEYWORDS = [b"ab", b"a", b"dcb", b"\xc3\xa9", b"bcda"]
E_INVALID, E_DEVICE = 1, 2


def _docs(rng, n, hi):
    alphabet = np.frombuffer(b"ab\xc3\xa9" if hi else b"abcd", dtype=np.uint8)
    lens = rng.integers(8, 41, n)
    return [alphabet[rng.integers(0, 4, int(l))].tobytes() for l in lens]


def pack(docs):
    blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    return blob, ds


def build_index(ids, docs, device=0):
    g = capi.GpuStringIndex(device=device)
    blob, ds = pack(docs)
    g.add_bulk(np.asarray(ids, dtype=np.int64), blob, ds)
    g.build()
    return g


def build_column(kind, ids, values, device=0):
    c = capi.GpuColumn(kind, device=device)
    if len(ids):
        c.add_bulk(ids, values)
    c.build()
    return c


# the model's inputs, made once and never changed
def _inputs(hi):
    rng = np.random.default_rng(20261020 + int(hi))
    strings = {"A": (IDS.copy(), _docs(rng, N, hi)), "B": (IDS[::2].copy(), _docs(rng, len(IDS[::2]), False))}
    c_ids = rng.permutation(IDS)[: N // 3]
    strings["C"] = (c_ids, _docs(rng, len(c_ids), False))
    held = rng.permutation(IDS[np.arange(N) % 5 != 0])
    levels = rng.integers(-40, 40, len(held))
    return strings, {name: (kind, held.copy(), CR.values_of(kind, levels)) for name, kind in (("b", 0), ("i", 1), ("d", 2))}


INPUTS = {False: _inputs(False), True: _inputs(True)}


class Db:
    """handles + model"""

    def __init__(self, hi=False, device=0):
        strings, columns = INPUTS[hi]
        self.hi = hi
        self.docs = {k: (ids.copy(), list(docs)) for k, (ids, docs) in strings.items()}
        self.idx = {k: build_index(ids, docs, device) for k, (ids, docs) in strings.items()}
        self.ref, self.col = {}, {}
        for k, (kind, ids, values) in columns.items():
            self.ref[k] = CR.RefColumn(kind)
            self.ref[k].build(ids, values)
            self.col[k] = build_column(kind, ids, values, device)

    def close(self):
        for h in list(self.idx.values()) + list(self.col.values()):
            h.close()

    def handles(self, names="ABCbid"):
        return [self.idx[k] if k in self.idx else self.col[k] for k in names]

    def model_remove(self, names, ids):
        """what every field of `names` reports, the model updated"""
        ids = np.asarray(ids, dtype=np.int64)
        out = []
        for k in names:
            if k in self.idx:
                fid, fdocs = self.docs[k]
                gone = np.isin(fid, ids)
                self.docs[k] = (fid[~gone], [d for d, g in zip(fdocs, gone) if not g])
                out.append((int(gone.sum()), len(ids) - int(gone.sum())))
            else:
                out.append(self.ref[k].remove(ids))
        return out

    def snapshot(self):
        """every array a field serves from, as bytes"""
        snap = {k: (g.size, g.bits, g.mask, g.sa_width, g.sa().tobytes()) for k, g in self.idx.items()}
        snap.update({k: tuple(a.tobytes() for a in c.arrays()) for k, c in self.col.items()})
        return snap

    def check(self, names="ABCbid"):
        for k in names:
            if k in self.idx:
                g = self.idx[k]
                f = build_index(*self.docs[k])
                try:
                    assert (g.size, g.bits, g.mask, g.sa_width) == (f.size, f.bits, f.mask, f.sa_width), k
                    assert np.array_equal(g.sa(), f.sa()), k
                    for kw in KEYWORDS:
                        assert g.query(kw) == f.query(kw), (k, kw)
                finally:
                    f.close()
            else:
                c, ref = self.col[k], self.ref[k]
                assert c.stat("rows") == len(ref.ids), k
                for name, got, want in zip(("keys_v", "ids_v", "id_sorted", "vpos"), c.arrays(), ref.arrays()):
                    assert got.dtype == want.dtype and np.array_equal(got, want), (k, name)
                if ref.kind == 0 and len(ref.ids):
                    assert len(c.query_ids("false")) == ref.n_false


@pytest.fixture
def db():
    d = Db()
    yield d
    d.close()


def rowset_of(ids, device=0):
    ids = np.sort(np.asarray(ids, dtype=np.int64))
    return capi.debug_rowset_from_rows(ids, np.zeros(len(ids), dtype=np.int64), device=device)


def remove_and_check(d, ids, names="ABCbid"):
    with rowset_of(ids) as rs:
        rows, res = rs.remove(d.handles(names))
        want = d.model_remove(names, ids)
        assert rows == len(ids) == rs.size
        for k, r, w in zip(names, res, want):
            assert (r["removed"], r["missing"]) == w, k
            assert r["removed"] + r["missing"] == rows, k
            assert r["status"] == 0 and r["committed"] == int(w[0] > 0), k
        d.check(names)
        return rs.stat("removes"), res


# ---- set sizes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0, 1, 4095, 4096, 4097])
def test_set_sizes(db, size):
    rng = np.random.default_rng(size)
    ids = rng.choice(IDS, size, replace=False)
    calls, _ = remove_and_check(db, ids)
    assert calls == (1 if size else 0)
    if not size:   # an empty set counts no call in any field
        assert all(g.stat("removes") == 0 for g in db.idx.values()) and all(c.stat("removes") == 0 for c in db.col.values())


def test_first_and_last_document_of_a_field(db):
    c_ids = db.docs["C"][0]
    remove_and_check(db, [IDS[0], IDS[-1], c_ids[0], c_ids[-1]])


def test_set_nobody_holds(db):
    before = db.snapshot()
    calls, res = remove_and_check(db, [1, 2, 999, IDS[-1] + 1, 1 << 60, -5])
    assert calls == 1 and all(r["committed"] == 0 and r["removed"] == 0 for r in res)
    assert db.snapshot() == before
    assert all(g.stat("removes") == 0 for g in db.idx.values()) and all(c.stat("removes") == 0 for c in db.col.values())


def test_every_id_then_append(db):
    remove_and_check(db, IDS)
    assert all(g.size == 0 for g in db.idx.values()) and all(c.stat("rows") == 0 for c in db.col.values())
    new_ids = np.array([7, 5, 9], dtype=np.int64)
    new_docs = [b"abra", b"cadabra", b"ab"]
    for k, g in db.idx.items():
        assert g.append(new_ids, *pack(new_docs)) == 3
        db.docs[k] = (new_ids, new_docs)
    for k, c in db.col.items():
        vals = CR.values_of(db.ref[k].kind, [3, -2, 0])
        assert c.append(new_ids, vals) == db.ref[k].append(new_ids, vals) == 3
    db.check()


# ---- field states and refusals -----------------------------------------------------------------------------------------
def test_never_built_field_among_built_ones(db):
    g0, c0 = capi.GpuStringIndex(device=0), capi.GpuColumn(1, device=0)
    try:
        ids = IDS[5:500:3]
        with rowset_of(ids) as rs:
            rows, res = rs.remove([db.idx["A"], g0, db.col["i"], c0])
        want = db.model_remove("Ai", ids)
        assert [(r["removed"], r["missing"]) for r in res] == [want[0], (0, rows), want[1], (0, rows)]
        assert [r["committed"] for r in res] == [1, 0, 1, 0] and all(r["status"] == 0 for r in res)
        assert g0.sa_width == 0 and c0.stat("rows") == 0
        db.check()
    finally:
        g0.close()
        c0.close()


def _refused(db, fields, match, ids=IDS[:100]):
    before = db.snapshot()
    with rowset_of(ids) as rs:
        with pytest.raises(capi.RowSetRemoveError, match=match) as e:
            rs.remove(fields)
        assert e.value.code == E_INVALID
        assert all((r["removed"], r["missing"], r["committed"]) == (0, 0, 0) for r in e.value.fields)
        assert rs.stat("removes") == 0
    assert db.snapshot() == before


def test_same_handle_twice_is_invalid(db):
    _refused(db, [db.idx["A"], db.col["i"], db.idx["A"]], None)
    _refused(db, [db.col["d"], db.col["d"]], None)


def test_column_with_staged_rows_refuses_the_whole_call(db):
    db.col["i"].add_bulk([5], [1])
    _refused(db, db.handles("ABid"), "rows were added since the last build")


def test_index_with_pending_additions_refuses_the_whole_call(db):
    db.idx["B"].add(5, b"pending")
    _refused(db, db.handles("AiB"), "documents were added since the last build")


def test_field_on_a_second_gpu_is_invalid(db):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = build_column(1, [1, 2], [3, 4], device=1)
    try:
        _refused(db, [db.idx["A"], other], "lives on another GPU")
    finally:
        other.close()


# ---- stats and equivalence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hi", [False, True])
def test_stats_of_the_set_and_of_every_field(hi):
    d = Db(hi=hi)
    try:
        ids = IDS[10:3000:2]
        with rowset_of(ids) as rs:
            rows, res = rs.remove(d.handles())
            want = d.model_remove("ABCbid", ids)
            assert (rs.stat("removes"), rs.stat("remove_fields")) == (1, 6) and rs.stat("remove_ms") > 0
            assert rs.stat("rows") == rows   # the set itself is left as it is
            _, _, _, missing = rs.cluster(d.col["i"])
            assert missing == rows           # ... its ids are simply no longer held
        for k, (removed, _) in zip("ABC", want):
            g = d.idx[k]
            rebuilt = hi and k == "A"        # the array in the reference's order is built over the compacted text
            assert (g.stat("removes"), g.stat("remove_compactions"), g.stat("remove_rebuilds")) == (1, int(not rebuilt), int(rebuilt)), k
            assert g.stat("remove_docs") == removed
        for k, (removed, _) in zip("bid", want[3:]):
            c = d.col[k]
            assert (c.stat("removes"), c.stat("remove_compactions"), c.stat("remove_rebuilds"), c.stat("remove_rows")) == (1, 1, 0, removed), k
        d.check()
    finally:
        d.close()


def test_equals_the_per_field_calls():
    old, new = Db(), Db()
    try:
        ids = np.sort(np.random.default_rng(3).choice(IDS, 5000, replace=False))
        with rowset_of(ids) as rs:
            down, _ = rs.rows()
            want = [h.remove(down) for h in old.handles()]
        with rowset_of(ids) as rs:
            _, res = rs.remove(new.handles())
        assert [(r["removed"], r["missing"]) for r in res] == want
        assert old.snapshot() == new.snapshot()
    finally:
        old.close()
        new.close()


def test_rows_of_a_real_filter(db):
    with capi.filter_rows([(db.idx["A"], [b"ab"]), (db.col["i"], "[-30,30]")]) as rs:
        ids, _ = rs.rows()
        assert 0 < len(ids) < N
        rows, res = rs.remove(db.handles())
    want = db.model_remove("ABCbid", ids)
    assert rows == len(ids) and [(r["removed"], r["missing"]) for r in res] == want
    assert res[0]["removed"] == rows and res[4]["removed"] == rows   # the two fields that made the set held every row
    db.check()


# ---- all or none -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", [0, 1, 2])
@pytest.mark.parametrize("names", ["ABC", "bid"])
def test_a_failed_prepare_changes_nothing(db, names, position):
    fields = sorted(db.handles(names), key=lambda h: h._h.value)   # address order
    victim = fields[position]
    ids = IDS[3:9000:5]   # (every field holds some of them, so every field has a change to prepare)
    before = db.snapshot()
    victim.set_option("debug_fail_prepare", 1)
    with rowset_of(ids) as rs:
        in_use = None
        for _ in range(2):   # the first failure warms the fields' kept work spaces and id tables; from then on in-use must not move
            with pytest.raises(capi.RowSetRemoveError, match=r"^field %d: debug: prepare failure requested" % position) as e:
                rs.remove(fields)
            assert e.value.code == E_DEVICE and e.value.rows == len(ids)
            assert [r["status"] for r in e.value.fields] == [E_DEVICE if k == position else 0 for k in range(3)]
            assert all((r["removed"], r["missing"], r["committed"]) == (0, 0, 0) for r in e.value.fields)
            assert db.snapshot() == before
            now = capi.memory_stats()[0]
            assert in_use is None or now == in_use
            in_use = now
        assert rs.stat("removes") == 0
        assert all(h.stat("removes") == 0 for h in fields)
        victim.set_option("debug_fail_prepare", 0)
        rows, res = rs.remove(fields)
    order = "".join(k for h in fields for k in names if (db.idx.get(k) or db.col.get(k)) is h)
    want = db.model_remove(order, ids)
    assert [(r["removed"], r["missing"]) for r in res] == want and all(r["committed"] == 1 for r in res)
    db.check()


def test_the_step_behind_the_commit():
    d = Db(hi=True)
    try:
        ids = IDS[100:2000]
        d.idx["A"].set_option("debug_fail_build", 1)
        with rowset_of(ids) as rs:
            with pytest.raises(capi.RowSetRemoveError, match=r"^field 1: debug: build failure requested") as e:
                rs.remove(d.handles("BAi"))
            assert rs.stat("removes") == 1
        want = d.model_remove("BAi", ids)
        res = e.value.fields
        assert e.value.code == E_INVALID and [r["status"] for r in res] == [0, E_INVALID, 0]
        assert [r["committed"] for r in res] == [1, 1, 1]
        assert [(r["removed"], r["missing"]) for r in res] == want
        assert d.idx["A"].sa_width == 0 and d.idx["A"].query(b"ab") == []   # never built
        d.check("BCbid")
    finally:
        d.close()


# ---- beside readers ----------------------------------------------------------------------------------------------------
def test_readers_see_before_or_after(db):
    A, col = db.idx["A"], db.col["i"]
    ids = IDS[::2]

    def answers():
        with capi.filter_rows([(A, [b"ab"]), (col, "[-30,30]")]) as f:
            both = f.rows()[0].tobytes()
        return A.query(b"dcb"), col.query_ids("[-30,30]").tobytes(), both

    before = answers()
    seen, stop, errors = [[], [], []], threading.Event(), []

    def reader(which):
        try:
            while not stop.is_set():
                if which == 0:
                    seen[0].append(A.query(b"dcb"))
                elif which == 1:
                    seen[1].append(col.query_ids("[-30,30]").tobytes())
                else:
                    with capi.filter_rows([(A, [b"ab"]), (col, "[-30,30]")]) as f:
                        seen[2].append(f.rows()[0].tobytes())
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=reader, args=(w,), daemon=True) for w in range(3)]
    for t in threads:
        t.start()
    try:
        remove_and_check(db, ids)
    finally:
        stop.set()
        for t in threads:
            t.join(30)
    assert not any(t.is_alive() for t in threads), "a reader did not come back"
    assert not errors, errors
    after = answers()
    for w in range(3):
        assert before[w] != after[w]
        assert all(a == before[w] or a == after[w] for a in seen[w]), w
