"""cdb_column_append and cdb_column_remove on the device (column_maintain.hip) against tests/column_referee.py: after every call
the four device arrays equal the referee's exactly, and the column answers like a fresh one built from the same final rows —
arrays, stats, query, query_any on both union paths, cluster on both paths (asked before the call too: the run table of the old
generation must not survive) and one cdb_query_and_columns.  Every case runs with debug_maintain_path 1 (device) and 2 (the
host filter / stage + build), for every kind the case allows."""
import numpy as np
import pytest

from coffeedb_amd import capi
from tests import column_referee as R

pytestmark = pytest.mark.gpu

APPEND = R.append_cases()   # made once, never changed
REMOVE = R.remove_cases()
RANGES = {1: ["[-30,30]", "(0,inf]"], 2: ["[-7.5,7.5]", "[-1000000,1000000]"], 0: ["false", "true"]}
PATHS = (1, 2)


def _kinds(cases):
    return [(name, kind) for name, c in cases.items() for kind in c[0]]


def _column(kind, ids, values, path):
    col = capi.GpuColumn(kind, device=0)
    col.set_option("debug_maintain_path", path)
    if len(ids):
        col.add_bulk(ids, values)
        col.build()
    return col


def _sample(ref):
    ids = ref.ids
    pick = ids if len(ids) <= 600 else ids[:: len(ids) // 500]
    return np.concatenate([np.sort(pick), [np.int64(1) << 60]]).astype(np.int64)   # (one id nobody holds)


def _clusters(col, ids):
    out = []
    for path in (1, 2):
        col.set_option("debug_cluster_path", path)
        v, c, r, miss = col.cluster(ids)
        out.append((v.tolist(), c.tolist(), r.tolist(), miss))
    col.set_option("debug_cluster_path", 0)
    return out


def _assert_arrays(col, ref):
    assert col.stat("rows") == len(ref.ids) and col.stat("kind") == ref.kind
    for name, got, want in zip(("keys_v", "ids_v", "id_sorted", "vpos"), col.arrays(), ref.arrays()):
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    if ref.kind == 0 and len(ref.ids):
        assert len(col.query_ids("false")) == ref.n_false


def _assert_like_fresh(col, ref):
    _assert_arrays(col, ref)
    fresh = _column(ref.kind, ref.ids, ref.values, 0)
    try:
        if not len(ref.ids):
            fresh.build()
        for a, b in zip(col.arrays(), fresh.arrays()):
            assert np.array_equal(a, b)
        rows = _sample(ref)
        for rng in RANGES[ref.kind]:
            assert np.array_equal(col.query_ids(rng), fresh.query_ids(rng)), rng
        for qp in (1, 2):
            col.set_option("debug_query_path", qp)
            fresh.set_option("debug_query_path", qp)
            assert np.array_equal(col.query_any(RANGES[ref.kind]), fresh.query_any(RANGES[ref.kind]))
        col.set_option("debug_query_path", 0)
        assert _clusters(col, rows) == _clusters(fresh, rows)
        host = [(int(i), 1) for i in rows]
        key = RANGES[ref.kind][:1]
        assert capi.query_and([(None, host), (col, key)]) == capi.query_and([(None, host), (fresh, key)])
    finally:
        fresh.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,kind", _kinds(APPEND))
def test_append(name, kind, path):
    _, oi, ol, ni, nl = APPEND[name]
    ref = R.RefColumn(kind)
    ref.build(oi, R.values_of(kind, ol))
    col = _column(kind, oi, R.values_of(kind, ol), path)   # (no rows: a column that was never built)
    try:
        _clusters(col, _sample(ref))
        concat = ref.id_concat(ni)
        assert col.append(ni, R.values_of(kind, nl)) == ref.append(ni, R.values_of(kind, nl)) == len(ni)
        merged = path == 1 and len(oi) > 0
        assert (col.stat("appends"), col.stat("append_merges"), col.stat("append_rebuilds")) == (1, int(merged), int(not merged))
        assert col.stat("append_rows") == len(ni) and col.stat("append_id_concat") == int(merged and concat)
        _assert_like_fresh(col, ref)
    finally:
        col.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,kind", _kinds(REMOVE))
def test_remove(name, kind, path):
    _, ids, lv, gone = REMOVE[name]
    ref = R.RefColumn(kind)
    ref.build(ids, R.values_of(kind, lv))
    col = _column(kind, ids, R.values_of(kind, lv), path)
    try:
        _clusters(col, _sample(ref))
        want = ref.remove(gone)
        assert col.remove(gone) == want
        did = int(want[0] > 0)
        assert (col.stat("removes"), col.stat("remove_compactions"), col.stat("remove_rebuilds")) == \
            (did, did * int(path == 1), did * int(path == 2))
        if did:
            assert col.stat("remove_rows") == want[0]
        _assert_like_fresh(col, ref)
        if name == "everything":   # an append into the emptied column works (the build of the batch)
            assert col.append(ids[:500], R.values_of(kind, lv[:500])) == ref.append(ids[:500], R.values_of(kind, lv[:500]))
            assert col.stat("append_rebuilds") == 1
            _assert_like_fresh(col, ref)
    finally:
        col.close()


@pytest.mark.parametrize("path", PATHS)
def test_append_double_zeros(path):
    """+0.0 against -0.0: one key, the id decides — on both sides of the old rows."""
    ref = R.RefColumn(2)
    oi, ov = np.arange(200, dtype=np.int64) * 10, np.where(np.arange(200) % 2 == 0, 0.0, -0.0)
    ni, nv = np.concatenate([oi + 5, [-3, -2]]), np.concatenate([-ov, [-0.0, 0.0]])
    ref.build(oi, ov)
    col = _column(2, oi, ov, path)
    try:
        assert col.append(ni, nv) == ref.append(ni, nv)
        assert len(set(ref.arrays()[0].tolist())) == 1 and np.array_equal(ref.arrays()[1], np.sort(ref.ids))
        _assert_like_fresh(col, ref)
    finally:
        col.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_append_errors_leave_the_column_as_it_was(kind, path):
    rng = np.random.default_rng(7)
    ids, lv = np.arange(5000, dtype=np.int64) * 2, rng.integers(-40, 40, 5000)
    ref = R.RefColumn(kind)
    ref.build(ids, R.values_of(kind, lv))
    col = _column(kind, ids, R.values_of(kind, lv), path)
    new = np.arange(300, dtype=np.int64) * 2 + 1
    nv = R.values_of(kind, rng.integers(-40, 40, 300))
    try:
        with_old = new.copy()
        with_old[137] = ids[4000]
        with pytest.raises(RuntimeError, match=rf"^cdb_column_append: duplicate object id {ids[4000]} in one column$"):
            col.append(with_old, nv)
        _assert_arrays(col, ref)
        twice = new.copy()
        twice[200] = twice[10]
        with pytest.raises(RuntimeError, match=rf"^cdb_column_append: duplicate object id {twice[10]} in one column$"):
            col.append(twice, nv)
        _assert_arrays(col, ref)
        if kind == 2:
            bad = nv.copy()
            bad[17] = np.nan
            with pytest.raises(RuntimeError, match=r"^cdb_column_append: NaN is not a valid value \(row 17\)$"):
                col.append(new, bad)
            _assert_arrays(col, ref)
        col.add_bulk(new[:5], nv[:5])   # pending staged rows
        with pytest.raises(RuntimeError, match=r"^append: rows were added since the last build$"):
            col.append(new[5:], nv[5:])
        assert col.stat("staged_rows") == 5 and col.stat("appends") == 0
        _assert_arrays(col, ref)
        col.build()
        ref.append(new[:5], nv[:5])
        assert col.append(new[:0], nv[:0]) == 0 and col.stat("appends") == 0   # n = 0 changes nothing
        assert col.append(new[5:], nv[5:]) == ref.append(new[5:], nv[5:])
        _assert_like_fresh(col, ref)
    finally:
        col.close()


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_remove_with_staged_rows_takes_the_host_path(kind):
    rng = np.random.default_rng(8)
    ids, lv = rng.permutation(6000).astype(np.int64), rng.integers(-40, 40, 6000)
    vals = R.values_of(kind, lv)
    ref = R.RefColumn(kind)
    ref.build(ids[:5000], vals[:5000])
    col = _column(kind, ids[:5000], vals[:5000], 1)
    try:
        col.add_bulk(ids[5000:], vals[5000:])
        ref.append(ids[5000:], vals[5000:])
        gone = np.concatenate([ids[100:400], ids[5500:5600], [-1]])   # built rows, staged rows, one nobody holds
        assert col.remove(gone) == ref.remove(gone) == (400, 1)
        assert (col.stat("removes"), col.stat("remove_compactions"), col.stat("remove_rebuilds")) == (1, 0, 1)
        _assert_like_fresh(col, ref)
    finally:
        col.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_sequence_append_remove_append_remove(kind, path):
    rng = np.random.default_rng(9)
    ids, lv = rng.permutation(20000).astype(np.int64) - 3000, rng.integers(-40, 40, 20000)
    vals = R.values_of(kind, lv)
    ref = R.RefColumn(kind)
    ref.build(ids[:9000], vals[:9000])
    col = _column(kind, ids[:9000], vals[:9000], path)
    try:
        assert col.append(ids[9000:14000], vals[9000:14000]) == ref.append(ids[9000:14000], vals[9000:14000])
        _assert_like_fresh(col, ref)
        gone = np.concatenate([ids[8000:10000], ids[15000:15010]])
        assert col.remove(gone) == ref.remove(gone) == (2000, 10)
        _assert_like_fresh(col, ref)
        assert col.append(ids[14000:], vals[14000:]) == ref.append(ids[14000:], vals[14000:])
        _assert_like_fresh(col, ref)
        assert col.remove(ids[::3]) == ref.remove(ids[::3])
        _assert_like_fresh(col, ref)
        assert col.remove(np.array([1 << 50])) == (0, 1)   # nothing dropped: not counted
        merges, rebuilds = (2, 0) if path == 1 else (0, 2)
        assert (col.stat("appends"), col.stat("append_merges"), col.stat("append_rebuilds")) == (2, merges, rebuilds)
        assert (col.stat("removes"), col.stat("remove_compactions"), col.stat("remove_rebuilds")) == (2, merges, rebuilds)
        assert col.stat("append_rows") == 6000 and col.stat("append_ms") > 0 and col.stat("remove_ms") > 0
    finally:
        col.close()


def test_profile_names_the_kernels():
    ids = np.arange(9000, dtype=np.int64) * 2
    col = _column(1, ids, ids % 17, 1)
    try:
        col.set_option("profile", 1)
        col.append(ids[:100] + 1, ids[:100] % 5)
        col.remove(ids[::7])
        names = set(col.profile())
        assert {"col_ap_rank", "col_ap_flag", "col_ap_count", "col_ap_value", "col_ap_id"} <= names
        assert {"col_rm_mark", "col_rm_count", "col_rm_value", "col_rm_id"} <= names
    finally:
        col.close()
