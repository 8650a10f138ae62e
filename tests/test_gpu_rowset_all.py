"""cdb_rowset_all (capi.rowset_all): the row set of every object — the union of the ids the given fields hold, ascending as signed
int64, each id once, every count 0 — against tests/rowset_all_referee.py (np.unique over the concatenated lists), and the
operations that then run over such a set unchanged: size, page on both paths, select, cluster, remove.  Exact equality everywhere.
The input sizes sit on the edges of the 4096-slot tiles of stable_tiles.h."""
import numpy as np
import pytest

from coffeedb_amd import capi

from . import rowset_all_referee as R
from . import select_referee as S

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EDGE = np.array([I64_MIN, -1, 0, I64_MAX], dtype=np.int64)
SELECT, SORT = 1, 2


def index_of(ids, shuffle=False, seed=0):
    """a string index holding `ids`; shuffle: inserted in an order that does not ascend (the id table is then a sorted copy)"""
    ids = np.asarray(ids, dtype=np.int64)
    if shuffle:
        ids = np.random.default_rng(seed).permutation(ids)
    docs = [b"doc %d" % (int(i) % 97) for i in ids]
    g = capi.GpuStringIndex(device=0)
    blob = np.frombuffer(b"".join(docs), dtype=np.uint8)
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    g.add_bulk(ids, blob, ds)
    g.build()
    return g, dict(zip(ids.tolist(), docs))


def column_of(ids, kind=1, seed=0):
    ids = np.random.default_rng(seed).permutation(np.asarray(ids, dtype=np.int64))
    vals = (ids % 7).astype(np.int64) if kind == 1 else (ids % 2 == 0)
    c = capi.GpuColumn(kind, device=0)
    if len(ids):
        c.add_bulk(ids, vals)
    c.build()
    return c, dict(zip(ids.tolist(), vals.tolist()))


def check_union(fields, lists):
    want = R.union(lists)
    with capi.rowset_all(fields) as rs:
        ids, counts = rs.rows()
        assert rs.size == len(want)
        assert ids.dtype == np.int64 and np.array_equal(ids, want)
        assert not counts.any() and len(counts) == len(want)
        assert (rs.stat("all_fields"), rs.stat("all_input_rows")) == (len(fields), sum(len(l) for l in lists))
    return want


def split(total, k, overlap, rng):
    """k id lists of `total` entries together, drawn from a pool around 0 (negative ids in it); overlap: the lists share ids"""
    pool = np.arange(-total, 2 * total, dtype=np.int64) * 5
    cut = [total * j // k for j in range(k + 1)]
    if overlap:
        return [np.sort(rng.choice(pool[: max(total, 4)], cut[j + 1] - cut[j], replace=False)) for j in range(k)]
    perm = rng.permutation(pool)[:total]
    return [np.sort(perm[cut[j]:cut[j + 1]]) for j in range(k)]


# ---- the union against the referee ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("k,total", [(k, t) for k in (1, 2, 3) for t in (1, 4095, 4096, 4097, 2 * 4096 + 1) if t >= k])
def test_union_of_k_fields(k, total, overlap):
    rng = np.random.default_rng(1000 * k + total + int(overlap))
    lists = split(total, k, overlap, rng)
    made = [index_of(l, shuffle=(j == 2), seed=j)[0] if j % 2 == 0 else column_of(l, seed=j)[0] for j, l in enumerate(lists)]   # index, column, index
    try:
        check_union(made, lists)
    finally:
        for h in made:
            h.close()


def test_run_of_equal_ids_across_a_tile_edge():
    """sorted input: 4094 distinct ids, then one id three times in slots 4094 .. 4096 (a run across 4095 | 4096), then more"""
    a = np.arange(4095, dtype=np.int64) * 2          # slots 0 .. 4094: the last one is 8188
    b = np.array([8188, 8190], dtype=np.int64)       # 8188 again: slot 4095
    c = np.concatenate([[8188], np.arange(8192, 8192 + 300, dtype=np.int64)])   # ... and slot 4096
    made = [index_of(a)[0], column_of(b)[0], column_of(c, kind=0)[0]]
    try:
        want = check_union(made, [a, b, c])
        assert (want == 8188).sum() == 1
    finally:
        for h in made:
            h.close()


def test_equal_lists_and_disjoint_lists():
    ids = np.arange(-3000, 3000, dtype=np.int64) * 3
    same = [index_of(ids)[0], column_of(ids)[0], index_of(ids, shuffle=True)[0]]
    apart = [index_of(ids[:2000])[0], column_of(ids[2000:4000])[0], column_of(ids[4000:], kind=0)[0]]
    try:
        assert len(check_union(same, [ids, ids, ids])) == len(ids)
        assert len(check_union(apart, [ids[:2000], ids[2000:4000], ids[4000:]])) == len(ids)
    finally:
        for h in same + apart:
            h.close()


def test_never_built_fields():
    g0, c0 = capi.GpuStringIndex(device=0), capi.GpuColumn(1, device=0)
    ids = np.arange(50, dtype=np.int64)
    g, _ = index_of(ids)
    try:
        check_union([g0, g, c0], [[], ids, []])
        check_union([g0, c0], [[], []])          # all never built: a valid set of size 0
        check_union([c0], [[]])
        with capi.rowset_all([g0]) as rs:
            assert rs.size == 0 and len(rs.page(0, 10)[0]) == 0
        c0.add_bulk([7], [1])                    # staged, not built: only built rows count
        check_union([c0, g], [[], ids])
    finally:
        for h in (g0, c0, g):
            h.close()


@pytest.mark.parametrize("k", [1, 2])
def test_extreme_ids_negative_first(k):
    a = np.concatenate([EDGE, [5, -7]]).astype(np.int64)
    b = np.array([I64_MAX, I64_MIN, -2, 3], dtype=np.int64)
    made = [index_of(a, shuffle=True)[0]] + ([column_of(b)[0]] if k == 2 else [])
    try:
        want = check_union(made, [a, b][:k])
        assert want[0] == I64_MIN and want[-1] == I64_MAX and list(want).index(-1) < list(want).index(0)
    finally:
        for h in made:
            h.close()


def test_index_whose_ids_do_not_ascend_alone():
    ids = np.arange(5000, dtype=np.int64) * 3 - 7000
    g, _ = index_of(ids, shuffle=True, seed=5)
    try:
        check_union([g], [ids])
    finally:
        g.close()


# ---- over the resulting set ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def database():
    ids = np.arange(-2500, 2500, dtype=np.int64) * 3
    g, docs = index_of(ids[::2])
    c, vals = column_of(ids[1::3])
    yield g, docs, c, vals, R.union([ids[::2], ids[1::3]])
    g.close()
    c.close()


@pytest.mark.parametrize("path", [SELECT, SORT])
def test_page_is_the_ascending_slice(database, path):
    g, _, c, _, want = database
    with capi.rowset_all([g, c]) as rs:
        rs.set_option("debug_page_path", path)
        for first, last in ((0, 10), (0, 1), (17, 300), (len(want) - 3, len(want)), (len(want) - 3, len(want) + 50), (5, 5), (len(want), len(want) + 1),
                            (0, len(want))):
            ids, counts = rs.page(first, last)
            wi, wc = R.page(want, first, last)
            assert np.array_equal(ids, wi) and np.array_equal(counts, wc), (first, last)
        assert rs.stat("page_selects" if path == SELECT else "page_sorts") > 0


def test_select_and_cluster_over_the_set(database):
    g, docs, c, vals, want = database
    with capi.rowset_all([g, c]) as rs:
        ids, counts, (text, values) = rs.select(40, 140, [(g, [b"doc"]), c], left=b"<", right=b">")
        page = want[40:140]
        assert np.array_equal(ids, page) and not counts.any()
        wt, wf, wm = S.field_text(docs, page, [b"doc"], b"<", b">")
        assert (text[0], text[1].tolist(), text[2]) == (wt, wf, wm)
        wv, wf, wm = S.field_values(vals, page)
        assert (values[0].tolist(), values[1].tolist(), values[2]) == (wv, wf, wm)
        cv, cc, cr, missing = rs.cluster(c)
        held = [i for i in want.tolist() if i in vals]
        groups = sorted(set(vals[i] for i in held))
        assert cv.tolist() == groups and missing == len(want) - len(held)
        assert cc.tolist() == [sum(1 for i in held if vals[i] == v) for v in groups]
        assert cr.tolist() == [min(i for i in held if vals[i] == v) for v in groups]


def test_remove_of_the_whole_set_empties_every_field():
    ids = np.arange(-4100, 4100, dtype=np.int64)
    g, _ = index_of(ids[::2], shuffle=True)
    c, _ = column_of(ids[::3])
    try:
        with capi.rowset_all([g, c]) as rs:
            rows, res = rs.remove([g, c])
            assert rows == len(R.union([ids[::2], ids[::3]]))
            assert [(r["removed"], r["missing"]) for r in res] == [(len(ids[::2]), rows - len(ids[::2])), (len(ids[::3]), rows - len(ids[::3]))]
        assert g.size == 0 and c.stat("rows") == 0
        with capi.rowset_all([g, c]) as rs:
            assert rs.size == 0
    finally:
        g.close()
        c.close()


def test_profile_lines_follow_the_lead(database):
    g, _, c, _, _ = database
    g.set_option("profile", 1)
    try:
        with capi.rowset_all([g, c]) as rs:
            prof = rs.profile()
            assert {"all_keys", "all_count", "all_unique"} <= set(prof) and rs.stat("all_ms") > 0
    finally:
        g.set_option("profile", 0)
