"""Select on the device (cdb_column_values, cdb_rowset_select; capi.GpuColumn.values, capi.GpuRowSet.select) — every comparison is
exact equality.  A column's referee is a Python dict; a select's is tests/select_referee.py over the same dicts plus
tests/rowset_referee.py for the page, and every string field must also equal render_rows of the same page ids.  Sizes sit at the
kernel's edges (lane 64, workgroup 256, one row past 4096), not at a workload's.

TIES: the reference ranks with std::sort and a comparator that ignores ids, so equal counts are unordered there; the project's
rule is ties ascending by id, and that rule is what the pages here are compared with."""
import numpy as np
import pytest

from coffeedb_amd import capi

from . import rowset_referee as R
from . import select_referee as S

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DBL_MAX = np.finfo(np.float64).max
SELECT, SORT = 1, 2
COLUMN_SIZES = [1, 2, 3, 255, 256, 257, 4097]
PAGE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257]
KINDS = [("int64", None), ("double", None), ("bool", "true"), ("bool", "false"), ("bool", "mixed")]


# ---- 1. cdb_column_values ------------------------------------------------------------------------------------------------
def column_rows(kind, variant, n, seed):
    """(ids, values): ids three apart (so there is an id between two held ones), given in DESCENDING order: rank != insertion index"""
    rng = np.random.default_rng(seed)
    ids = (np.arange(n, dtype=np.int64) * 3 - (3 * n) // 2)[::-1].copy()
    if kind == "int64":
        vals = rng.integers(-1000, 1000, n).astype(np.int64)
        edge = np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64)
    elif kind == "double":
        vals = rng.standard_normal(n)
        edge = np.array([-0.0, np.inf, -np.inf, 5e-324, DBL_MAX, -DBL_MAX, 0.0], dtype=np.float64)
    else:
        vals = {"true": np.ones(n, dtype=bool), "false": np.zeros(n, dtype=bool), "mixed": rng.integers(0, 2, n).astype(bool)}[variant]
        edge = vals[:0]
    k = min(n, len(edge))
    vals[:k] = rng.permutation(edge)[:k]
    return ids, vals


def raw_bits(kind, v):
    """the uint64 the library returns for a value of the model (-0.0 was folded onto +0.0 when the column was built)"""
    if kind == "int64":
        return int(v) & 0xFFFFFFFFFFFFFFFF
    if kind == "double":
        return int(np.array([float(v) + 0.0], dtype=np.float64).view(np.uint64)[0])
    return int(bool(v))


def questions(held, p, seed):
    """p ids to ask for: the edges first (for p >= 8 all of them), then held and unheld ids at random, one of them repeated"""
    lo, hi = min(held), max(held)
    ask = [lo - 1, hi + 1, lo + 1, lo, hi, I64_MIN, I64_MAX, lo]
    rng = np.random.default_rng(seed)
    pool = np.array(sorted(held), dtype=np.int64)
    while len(ask) < p:
        ask.append(int(pool[rng.integers(0, len(pool))]) + int(rng.integers(0, 2)))   # (+1: between two held ids, or just past the last)
    if p == 1:
        ask = [hi]
    return np.array(ask[:p], dtype=np.int64)


def check_values(col, kind, model, what):
    dtype = {"int64": np.int64, "double": np.float64, "bool": np.bool_}[kind]
    held = model if model else {0: 0}
    for p in PAGE_SIZES:
        ask = questions(held, p, p)
        values, found, missing = col.values(ask, with_missing=True)
        assert values.dtype == dtype and len(values) == p and len(found) == p, (what, p)
        want_found = [int(i) in model for i in ask]
        want_raw = [raw_bits(kind, model[int(i)]) if int(i) in model else 0 for i in ask]
        got_raw = values.view(np.uint64).tolist() if kind != "bool" else values.astype(np.uint64).tolist()
        assert found.tolist() == want_found, (what, p)
        assert got_raw == want_raw, (what, p)
        assert missing == want_found.count(False), (what, p)
        bits, found2 = col.values(ask, raw=True)       # the uint64 of the C side: a bool is exactly 0 or 1
        assert bits.dtype == np.uint64 and bits.tolist() == want_raw and found2.tolist() == want_found, (what, p, "raw")


@pytest.mark.parametrize("kind,variant", KINDS, ids=[k + ("_" + v if v else "") for k, v in KINDS])
def test_column_values_edges(kind, variant):
    for n in COLUMN_SIZES:
        ids, vals = column_rows(kind, variant, n, 100 + n)
        col = capi.GpuColumn(kind, device=0)
        check_values(col, kind, {}, (kind, variant, n, "never built"))
        col.add_bulk(ids, vals)
        check_values(col, kind, {}, (kind, variant, n, "staged, not built"))   # rows staged since the last build are not seen
        col.build()
        model = {int(i): v for i, v in zip(ids, vals.tolist())}
        check_values(col, kind, model, (kind, variant, n, "built"))
        # vpos is rewritten by both: new rows between the old ids (and behind them), then every third old row leaves
        new_ids = np.concatenate([ids[: (n + 1) // 2] + 1, [int(ids.max()) + 50]]).astype(np.int64)
        _, new_vals = column_rows(kind, variant, len(new_ids), 7 * n)
        assert col.append(new_ids, new_vals) == len(new_ids)
        model.update({int(i): v for i, v in zip(new_ids, new_vals.tolist())})
        check_values(col, kind, model, (kind, variant, n, "appended"))
        gone = sorted(model)[::3]
        assert col.remove(np.array(gone, dtype=np.int64)) == (len(gone), 0)
        for i in gone:
            del model[i]
        check_values(col, kind, model, (kind, variant, n, "removed"))
        col.close()


def test_column_values_profile_names_the_kernel():
    col = capi.GpuColumn("int64", device=0)
    col.add_bulk(np.arange(300, dtype=np.int64), np.arange(300, dtype=np.int64) * 2)
    col.build()
    col.set_option("profile", 1)
    values, found = col.values(np.arange(-5, 295, dtype=np.int64))
    assert values[5:].tolist() == (np.arange(295) * 2).tolist() and found.tolist() == [False] * 5 + [True] * 295
    assert col.profile()["sel_values"]["launches"] == 1


# ---- 2. cdb_rowset_select --------------------------------------------------------------------------------------------------
UNIVERSE = 4200
KW_SECRET, KW_NAME = [b"010", b"3", b"00"], [b"ab", b"b", b"abc"]
LEFT, RIGHT = b"<b>", b"</b>"


def build_index(ix, ids, docs):
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    ix.add_bulk(ids, np.frombuffer(b"".join(docs) or b"\0", dtype=np.uint8), ds)
    ix.build()


class World:
    """the fields of the tests below over one universe of ids, each with its dict model"""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.ids = np.arange(UNIVERSE, dtype=np.int64) * 5 - 9000
        k = np.arange(UNIVERSE)

        def docs(alphabet, n):
            out = []
            for _ in range(n):
                m = int(rng.integers(0, 25))
                out.append(bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), m).tolist()))
            return out

        # "secret": every id, ids ascending; empty documents among them
        d = docs(b"0103 ", UNIVERSE)
        d[0], d[5] = b"3010103", b""
        self.secret = capi.GpuStringIndex(0)
        build_index(self.secret, self.ids, d)
        self.m_secret = dict(zip(self.ids.tolist(), d))
        # "name": lacks every third id, and its ids do not ascend
        own = rng.permutation(self.ids[k % 3 != 0])
        d = docs(b"abc", len(own))
        self.name = capi.GpuStringIndex(0)
        build_index(self.name, own, d)
        self.m_name = dict(zip(own.tolist(), d))
        self.unbuilt = capi.GpuStringIndex(0)
        # the same "secret" documents as two shards on device 0
        self.shards = capi.GpuShards([0, 0])
        self.shards.set_option("use_all_devices", 1)
        build_index(self.shards, self.ids, [self.m_secret[int(i)] for i in self.ids])
        # five columns; the fourth lacks ids, the fifth was given its rows in descending id order
        self.columns, self.m_columns = [], []
        specs = [("int64", self.ids, rng.integers(-50, 50, UNIVERSE).astype(np.int64)),
                 ("double", self.ids, np.round(rng.standard_normal(UNIVERSE), 2)),
                 ("bool", self.ids, rng.integers(0, 2, UNIVERSE).astype(bool)),
                 ("int64", self.ids[k % 4 != 1], (k[k % 4 != 1] * 1000003).astype(np.int64)),
                 ("bool", self.ids[::-1].copy(), (k[::-1] % 5 == 0))]
        for kind, ids, vals in specs:
            col = capi.GpuColumn(kind, device=0)
            col.add_bulk(ids, vals)
            col.build()
            self.columns.append(col)
            self.m_columns.append((kind, dict(zip(ids.tolist(), vals.tolist()))))

    def fields(self):
        return ([(self.secret, KW_SECRET), (self.name, KW_NAME), (self.secret, []), (self.unbuilt, KW_SECRET)] + self.columns +
                [(self.shards, KW_SECRET)])

    def check(self, rs, ids, counts, first, last, what):
        """one select with every field, against the referee and against render_rows of the same page"""
        got_ids, got_counts, got = rs.select(first, last, self.fields(), LEFT, RIGHT)
        want_ids, want_counts = R.page(ids, counts, first, last)
        assert got_ids.tolist() == want_ids.tolist() and got_counts.tolist() == want_counts.tolist(), what
        page = want_ids
        strings = [(self.secret, self.m_secret, KW_SECRET), (self.name, self.m_name, KW_NAME), (self.secret, self.m_secret, []),
                   (self.unbuilt, {}, KW_SECRET)]
        for j, (ix, model, kws) in enumerate(strings):
            texts, found, missing = S.field_text(model, page, kws, LEFT, RIGHT)
            assert got[j][0] == texts and got[j][1].tolist() == found and got[j][2] == missing, (what, "string field", j)
            r_found, r_texts, _, r_missing = ix.render_rows(page, kws, LEFT, RIGHT, spans=False)
            assert got[j][0] == r_texts and got[j][1].tolist() == r_found.tolist() and got[j][2] == r_missing, (what, "render_rows", j)
        for j, (kind, model) in enumerate(self.m_columns):
            values, found, missing = S.field_values(model, page)
            g = got[len(strings) + j]
            assert g[0].dtype == capi.GpuColumn.DTYPES[capi.GpuColumn.KINDS[kind]] or kind == "bool", what
            assert g[0].tolist() == values and g[1].tolist() == found and g[2] == missing, (what, "column", j)
        texts, found, missing = S.field_text(self.m_secret, page, KW_SECRET, LEFT, RIGHT)
        g = got[-1]
        assert g[0] == texts and g[1].tolist() == found and g[2] == missing, (what, "shards")
        r_found, r_texts, _, r_missing = self.shards.render_rows(page, KW_SECRET, LEFT, RIGHT, spans=False)
        assert g[0] == r_texts and g[1].tolist() == r_found.tolist() and g[2] == r_missing, (what, "shards render_rows")
        return len(page)


@pytest.fixture(scope="module")
def world():
    return World()


def pages(m):
    return [(0, m), (0, 1), (m - 1, m), (m, m + 3), (m + 2, m + 9), (0, m + 7), (m // 2, m + 1)]


@pytest.mark.parametrize("m", [1, 2, 257, 4097])
def test_select_from_rows(world, m):
    rng = np.random.default_rng(m)
    ids = world.ids[:m].copy()
    if m > 2:
        ids[-1] = world.ids[-1] + 3          # an id no field holds
    counts = rng.integers(-2, 6, m).astype(np.int64)   # many ties, some negative counts
    with capi.debug_rowset_from_rows(ids, counts, device=0) as rs:
        selects = 0
        for forced in (SELECT, SORT):
            rs.set_option("debug_page_path", forced)
            for first, last in pages(m):
                before = (rs.stat("page_selects"), rs.stat("page_sorts"))
                n = world.check(rs, ids, counts, first, last, (m, forced, first, last))
                selects += 1
                k = min(last, m)
                sel, srt = rs.stat("page_selects") - before[0], rs.stat("page_sorts") - before[1]
                if first >= k:
                    assert (sel, srt) == (0, 0) and n == 0
                elif forced == SORT or k == m:
                    assert (sel, srt) == (0, 1)
                else:
                    assert (sel, srt) == (1, 0)
                assert rs.stat("selects") == selects and rs.stat("select_rows") == n and rs.stat("select_ms") > 0
                # nfields = 0 is cdb_rowset_page
                gi, gc, gf = rs.select(first, last, [])
                selects += 1
                pi, pc = rs.page(first, last)
                assert gi.tolist() == pi.tolist() and gc.tolist() == pc.tolist() and gf == []


def test_select_from_filter(world):
    """a row set cdb_filter made over a real string key plus a column"""
    # (an open lower bound: the reference's (value, id) bound pair makes a closed one skip NEGATIVE ids at the bound itself)
    with capi.filter_rows([(world.secret, [b"010"]), (world.columns[0], "(-21,30]")]) as rs:
        ids, counts = rs.rows()
        kind, values = world.m_columns[0]
        want = {}
        for i, doc in world.m_secret.items():
            occ = sum(1 for p in range(len(doc) - 2) if doc[p:p + 3] == b"010")
            if occ and -20 <= values[i] <= 30:
                want[i] = occ
        assert dict(zip(ids.tolist(), counts.tolist())) == want and len(want) > 300
        m = len(ids)
        for forced in (SELECT, SORT):
            rs.set_option("debug_page_path", forced)
            for first, last in ((0, m), (0, 1), (m - 1, m), (0, 10), (m, m + 1), (5, m + 5)):
                world.check(rs, ids, counts, first, last, ("filter", forced, first, last))


def test_select_raw_and_one_block(world):
    ids, counts = world.ids[:300], np.arange(300, dtype=np.int64) % 7
    with capi.debug_rowset_from_rows(ids, counts, device=0) as rs:
        rs.set_option("profile", 1)
        col = world.columns[3]
        gi, gc, got = rs.select(0, 100, [col, (world.name, KW_NAME), col, world.columns[1]], LEFT, RIGHT, raw=True)
        assert rs.profile()["sel_values"]["launches"] == 1          # three column fields, one launch
        page, _ = R.page(ids, counts, 0, 100)
        assert gi.tolist() == page.tolist()
        kind, model = world.m_columns[3]
        values, found, missing = S.field_values(model, page)
        for g in (got[0], got[2]):                                    # the same column twice
            assert g["kind"] == 1 and g["values"].view(np.int64).tolist() == values and g["found"].tolist() == found and g["missing"] == missing
        assert got[3]["kind"] == 2 and got[3]["values"].view(np.float64).tolist() == S.field_values(world.m_columns[1][1], page)[0]
        texts, found, missing = S.field_text(world.m_name, page, KW_NAME, LEFT, RIGHT)
        r = world.name.render_rows(page, KW_NAME, LEFT, RIGHT, spans=False, raw=True)
        assert got[1]["kind"] == 3 and got[1]["text_blob"] == b"".join(texts) == r["text_blob"]
        assert got[1]["text_ptr"].tolist() == r["text_ptr"].tolist() and got[1]["missing"] == missing == r["missing"]


def test_select_errors_leave_the_row_set_usable(world):
    ids, counts = world.ids[:50], np.arange(50, dtype=np.int64)
    with capi.debug_rowset_from_rows(ids, counts, device=0) as rs:
        with pytest.raises(RuntimeError, match="Empty keywords are not allowed"):
            rs.select(0, 10, [world.columns[0], (world.secret, [b"010", b""])])
        with pytest.raises(RuntimeError, match="Empty keywords are not allowed"):
            rs.select(0, 10, [(world.shards, [b""])])
        assert rs.stat("selects") == 0 and rs.stat("page_sorts") == 0     # refused before the page was made
        with pytest.raises(TypeError):
            rs.select(0, 10, [(world.columns[0], [])])
        assert world.check(rs, ids, counts, 0, 10, "after the failures") == 10


def test_select_field_on_another_device(world):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    other = capi.GpuColumn("int64", device=1)
    other.add_bulk(world.ids[:10], np.arange(10, dtype=np.int64))
    other.build()
    sx = capi.GpuStringIndex(1)
    build_index(sx, world.ids[:3], [b"a", b"b", b"c"])
    with capi.debug_rowset_from_rows(world.ids[:10], np.zeros(10, dtype=np.int64), device=0) as rs:
        for fields in ([other], [(sx, [])], [world.columns[0], other]):
            with pytest.raises(RuntimeError, match="another GPU"):
                rs.select(0, 5, fields)
        assert world.check(rs, world.ids[:10], np.zeros(10, dtype=np.int64), 0, 5, "after the refusals") == 5
