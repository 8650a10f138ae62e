"""Row sets on the GPU (cdb_filter, cdb_rowset_*; capi.filter_rows, capi.GpuRowSet) — every comparison is exact equality.
The page's referee is numpy (tests/rowset_referee.py): key = ~(count ^ 2^63), stable argsort, slice.  Sizes sit around the scan
tile (4096 rows) and the 256-thread workgroup; both page paths are forced and the counters prove which one ran."""
import re

import numpy as np
import pytest

from coffeedb_amd import capi, workloads as W

from . import rowset_referee as R

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TILE = 4096
SIZES = [1, 2, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 1]
SELECT, SORT = 1, 2
AUTO_SELECT_MIN_ROWS = 1 << 22   # rowset.hip: the automatic rule selects from this size on


def _boundary(m):
    """the row index a pattern is built around: the second scan tile's first row, else the second workgroup's, else the middle"""
    return TILE if m > TILE else (256 if m > 256 else m // 2)


def patterns(m):
    """name -> (counts, extra pages, select_passes the issue states or None)"""
    rng = np.random.default_rng(1000 + m)
    b = _boundary(m)
    out = {}
    out["equal"] = (np.full(m, 7, dtype=np.int64), [], 0)
    out["distinct"] = (rng.permutation(np.arange(m, dtype=np.int64)) * 1000003 - 17, [], None)
    two = np.full(m, 5, dtype=np.int64)
    two[b:] = 9
    out["two_values_split_at_tile"] = (two, [], 1 if 0 < b < m else 0)
    # a tie group that starts in one tile and ends in the next, and the page that ends inside it
    lo, hi = max(0, b - 10), min(m, b + 10)
    tie = np.full(m, 9, dtype=np.int64)
    tie[lo:hi] = 3
    tie[hi:] = 1
    k_tie = lo + (hi - lo) // 2 + 1   # the rows before the group outrank it, the rows behind it do not
    out["tie_group_across_tiles"] = (tie, [(0, k_tie), (k_tie - 1, k_tie), (max(0, k_tie - 3), k_tie + 1)], None)
    d5 = rng.integers(0, 256, m).astype(np.int64)
    out["byte_five_only"] = (0x1234 + (d5 << 40), [], 1 if len(set(d5.tolist())) > 1 else 0)
    pool = np.array([I64_MIN, -1, 0, 1, I64_MAX], dtype=np.int64)
    ext = pool[rng.integers(0, 5, m)]
    ext[:min(m, 5)] = pool[:min(m, 5)]
    out["extremes"] = (ext, [], 8 if m >= 2 else 0)
    # counts below 256: the threshold's digit is 0 where rank K - 1 holds count 255 (page (0, 1)), 255 where it holds count 0
    # (pages that end in the zeros at the tail of the ranking)
    edge = np.array([0, 255, 7, 100], dtype=np.int64)[rng.integers(0, 4, m)]
    edge[0] = 255
    edge[-1] = 0
    if m >= 3:
        edge[-2] = 0
    out["threshold_digit_zero_and_max"] = (edge, [], 1 if m >= 2 else 0)
    return out


def pages(m):
    p = [(0, 1), (0, m), (0, m - 1), (m - 1, m), (m // 2, m // 2), (m, m + 5), (m + 3, m + 9), (0, m + 7), (m // 3, m + 1), (m // 4, m // 2)]
    for k in (4095, 4096, 4097):
        if k <= m:
            p += [(0, k), (max(0, k - 300), k)]
    return [(f, l) for f, l in p if f >= 0 and l >= 0]


def check_page(rs, ids, counts, first, last, forced, stated_passes, what):
    m = len(ids)
    before = (rs.stat("page_selects"), rs.stat("page_sorts"))
    gi, gc = rs.page(first, last)
    wi, wc = R.page(ids, counts, first, last)
    assert gi.tolist() == wi.tolist() and gc.tolist() == wc.tolist(), what
    k = min(last, m)
    sel, srt = rs.stat("page_selects") - before[0], rs.stat("page_sorts") - before[1]
    if first >= k:
        assert (sel, srt) == (0, 0), what          # no rows: neither path runs
    elif forced == SORT or k == m or (forced == 0 and m < AUTO_SELECT_MIN_ROWS):
        assert (sel, srt) == (0, 1), what
    else:
        assert (sel, srt) == (1, 0), what
        assert rs.stat("select_passes") == R.differing_bytes(counts), what
        if stated_passes is not None:
            assert rs.stat("select_passes") == stated_passes, what


@pytest.mark.parametrize("m", SIZES)
def test_select_edges(m):
    ids = np.arange(m, dtype=np.int64) * 3 - 5 * m
    for name, (counts, extra, stated) in patterns(m).items():
        with capi.debug_rowset_from_rows(ids, counts, device=0) as rs:
            assert rs.size == m and rs.stat("rows") == m
            for forced in (SELECT, SORT, 0):
                rs.set_option("debug_page_path", forced)
                for first, last in pages(m) + extra:
                    check_page(rs, ids, counts, first, last, forced, stated, (m, name, forced, first, last))
            ri, rc = rs.rows()
            assert ri.tolist() == ids.tolist() and rc.tolist() == counts.tolist()


@pytest.mark.parametrize("m", [AUTO_SELECT_MIN_ROWS - 1, AUTO_SELECT_MIN_ROWS])
def test_automatic_rule_at_its_threshold(m):
    ids = np.arange(m, dtype=np.int64)
    counts = np.random.default_rng(m).integers(0, 1 << 20, m).astype(np.int64)
    with capi.debug_rowset_from_rows(ids, counts, device=0) as rs:
        for first, last in ((0, 100), (TILE - 1, TILE + 1), (0, m)):
            check_page(rs, ids, counts, first, last, 0, None, (m, first, last))
        assert rs.stat("page_selects") == (2 if m >= AUTO_SELECT_MIN_ROWS else 0)


def test_empty_row_set_and_options():
    with capi.debug_rowset_from_rows([], [], device=0) as rs:
        assert rs.size == 0
        for first, last in ((0, 0), (0, 1), (3, 9)):
            gi, gc = rs.page(first, last)
            assert len(gi) == 0 and len(gc) == 0
        assert rs.stat("page_selects") == 0 and rs.stat("page_sorts") == 0
        with pytest.raises(ValueError):
            rs.set_option("debug_page_path", 3)
        with pytest.raises(KeyError):
            rs.stat("no_such_stat")


def test_profile_names_the_page_kernels():
    m = 2 * TILE + 5
    ids = np.arange(m, dtype=np.int64)
    counts = np.random.default_rng(3).integers(0, 70000, m).astype(np.int64)
    with capi.debug_rowset_from_rows(ids, counts, device=0) as rs:
        rs.set_option("profile", 1)
        rs.set_option("debug_page_path", SELECT)
        rs.page(5, 100)
        prof = rs.profile()
        assert prof["pg_hist"]["launches"] == rs.stat("select_passes") == R.differing_bytes(counts)
        assert prof["pg_pick"]["launches"] == prof["pg_hist"]["launches"]
        assert prof["pg_hist"]["bytes"] == prof["pg_hist"]["launches"] * m * 8
        assert prof["pg_take"]["launches"] == 1 and prof["pg_out"]["launches"] == 1
        rs.set_option("debug_page_path", SORT)
        rs.page(5, 100)
        assert rs.profile()["pg_key"]["launches"] == 1 and rs.profile()["pg_out"]["launches"] == 2
        # a buffer the table does not fit is an error, not a shorter table
        import ctypes as C
        small = C.create_string_buffer(16)
        assert rs._lib.cdb_debug_rowset_profile_dump(rs._h, small, len(small)) == 1 and len(small.value) == 15


# ---- filter parity --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    n = 400
    rng = np.random.default_rng(77)
    ids = np.arange(n, dtype=np.int64) * 7 - 900
    blob, ds = W.ragged_corpus(n, 14, seed=5, lo=0x61, hi=0x64)   # short documents over "abcd"
    g = capi.GpuStringIndex(device=0)
    g.add_bulk(ids, blob, ds)
    g.build()
    ages = rng.integers(0, 100, n).astype(np.int64)
    active = rng.integers(0, 2, n).astype(np.uint8)
    age = capi.GpuColumn("int64", device=0)
    age.add_bulk(ids, ages)
    age.build()
    act = capi.GpuColumn("bool", device=0)
    act.add_bulk(ids, active)
    act.build()
    yield {"ids": ids, "blob": blob, "ds": ds, "g": g, "age": age, "act": act, "ages": ages, "active": active}
    for h in (age, act, g):
        h.close()


def check_filter(keys, corr):
    lo, hi = (I64_MIN, I64_MAX) if corr is None else corr
    plain = [r for r in capi.query_and(keys, ranked=False) if corr is None or lo <= r[1] < hi]
    ranked = capi.query_and(keys, ranked=True, lo=lo, hi=hi, limit=0)
    assert all(c >= 0 for _, c in plain)   # (the ranked call orders counts as unsigned: the two orders agree here)
    with capi.filter_rows(keys, corr) as rs:
        gi, gc = rs.rows()
        assert list(zip(gi.tolist(), gc.tolist())) == plain
        assert rs.size == len(plain) == len(rs)
        pi, pc = rs.page(0, rs.size)
        assert list(zip(pi.tolist(), pc.tolist())) == ranked
        ri, rc = R.ranking(gi, gc)
        assert pi.tolist() == ri.tolist() and pc.tolist() == rc.tolist()
        n = rs.size
        for path in (SELECT, SORT):
            rs.set_option("debug_page_path", path)
            for first, last in ((0, 1), (0, 10), (3, n // 2), (n // 2, n + 4), (n, n + 1)):
                qi, qc = rs.page(first, last)
                assert list(zip(qi.tolist(), qc.tolist())) == (ranked[first:last] if first < last else []), (path, first, last)
    return len(plain)


@pytest.mark.parametrize("corr", [None, (1, 1 << 62), (2, 4)])
def test_filter_parity(store, corr):
    g, age, act = store["g"], store["age"], store["act"]
    mat0, probe0 = age.stat("materialised_keys"), age.stat("probe_filters")
    assert check_filter([(g, [b"a", b"cd"]), (age, ["[10,12]"])], corr) > 0 or corr == (2, 4)   # a narrow column key: materialised
    assert age.stat("materialised_keys") > mat0
    check_filter([(g, [b"abc", b"dd"]), (age, ["[0,95]"])], corr)                                # a broad one: probes the merge
    assert age.stat("probe_filters") > probe0
    host = [(int(i), int(c)) for i, c in zip(store["ids"][::3], (np.arange(len(store["ids"][::3])) % 4))]
    check_filter([(g, [b"b"]), (None, host)], corr)                                              # a host-rows key
    check_filter([(g, [b"ab"]), (act, ["true"]), (age, ["[20,80]"])], corr)
    check_filter([(g, [b"a", b"b", b"c", b"d"])], corr)                                          # string key alone
    check_filter([(age, ["[30,60]"]), (act, ["false"])], corr)                                   # columns alone
    assert check_filter([(g, [b"a"]), (age, ["[50,40]"])], corr) == 0                            # empty intersection
    assert check_filter([(g, [b"zzzz"]), (act, ["true"])], corr) == 0


def test_filter_errors_are_those_of_query_and_on_the_same_handle(store):
    g, age, act = store["g"], store["age"], store["act"]
    lib = capi.load_library()
    cases = [([(g, [b"a", b""]), (age, ["[1,2]"])], "Empty keywords are not allowed", g),
             ([(g, []), (age, ["[1,2]"])], "The constraint list cannot be empty", g),
             ([(age, [])], "The constraint list cannot be empty", age),
             ([(g, [b"a"]), (age, ["1..2"])], "Invalid range: 1..2", g),
             ([(act, ["yes"])], 'Invalid query: "yes"', act)]
    for keys, text, handle in cases:
        last = lib.cdb_column_last_error if isinstance(handle, capi.GpuColumn) else lib.cdb_last_error
        with pytest.raises(RuntimeError, match=re.escape(text)) as e_and:
            capi.query_and(keys)
        on_handle_and = last(handle._h)
        with pytest.raises(RuntimeError, match=re.escape(text)) as e_filter:
            capi.filter_rows(keys, (1, 5))
        assert str(e_filter.value) == str(e_and.value)
        assert last(handle._h) == on_handle_and == str(e_and.value).encode()


# ---- ownership ------------------------------------------------------------------------------------------------------------------
def test_row_set_outlives_queries_rebuild_and_destruction():
    n = 300
    rng = np.random.default_rng(9)
    ids = np.arange(n, dtype=np.int64) * 11 + 4
    blob, ds = W.ragged_corpus(n, 12, seed=8, lo=0x61, hi=0x63)
    g = capi.GpuStringIndex(device=0)
    g.add_bulk(ids, blob, ds)
    g.build()
    age = capi.GpuColumn("int64", device=0)
    age.add_bulk(ids, rng.integers(0, 50, n))
    age.build()
    keys = [(g, [b"a", b"bc"]), (age, ["[5,40]"])]
    rs = capi.filter_rows(keys, (1, 1 << 62))
    assert rs.size > 10
    rows0 = [a.tolist() for a in rs.rows()]
    page0 = [a.tolist() for a in rs.page(2, 9)]
    # other queries through the handles that produced it (their q_ids / q_counts are overwritten)
    capi.query_and([(g, [b"c"]), (age, ["[0,3]"])], ranked=True)
    g.query(b"ab")
    other = capi.filter_rows([(g, [b"b"])])
    assert [a.tolist() for a in rs.rows()] == rows0
    # the index is rebuilt over more documents, the column is destroyed
    more, mds = W.ragged_corpus(50, 12, seed=3, lo=0x61, hi=0x63)
    g.add_bulk(np.arange(50, dtype=np.int64) + 10 ** 6, more, mds)
    g.build()
    age.close()
    assert [a.tolist() for a in rs.rows()] == rows0
    assert [a.tolist() for a in rs.page(2, 9)] == page0
    g.close()
    assert [a.tolist() for a in rs.page(2, 9)] == page0 and rs.size == len(rows0[0])
    other.close()
    rs.close()
    rs.close()   # closing twice is harmless


# ---- cluster parity -------------------------------------------------------------------------------------------------------------
def same_groups(a, b):
    va, ca, ra, ma = a
    vb, cb, rb, mb = b
    if isinstance(va, np.ndarray):
        assert va.dtype == vb.dtype and va.tobytes() == vb.tobytes()
    else:
        assert va == vb
    assert ca.tolist() == cb.tolist() and ra.tolist() == rb.tolist() and ma == mb


def test_cluster_parity(store):
    g, age, act, ids = store["g"], store["age"], store["act"], store["ids"]
    dbl = capi.GpuColumn("double", device=0)
    dbl.add_bulk(ids, np.round(np.random.default_rng(2).normal(0, 2, len(ids)), 0))
    dbl.build()
    strangers = np.array([ids[-1] + 1, ids[-1] + 50], dtype=np.int64)   # ids no field holds
    some = np.sort(np.concatenate([ids[5::2], strangers]))
    sets = [capi.debug_rowset_from_rows(some, np.ones(len(some)), device=0),
            capi.filter_rows([(g, [b"a", b"bd"]), (age, ["[0,70]"])], (1, 1 << 62)),
            capi.debug_rowset_from_rows([], [], device=0),               # empty
            capi.debug_rowset_from_rows(ids, np.arange(len(ids)), device=0)]   # dense enough for the counters-per-position path
    for rs in sets:
        rid = rs.rows()[0]
        for wv in (True, False):
            same_groups(rs.cluster(g, wv), g.cluster(rid, wv))
        for col in (age, act, dbl):
            for path in (1, 2):
                col.set_option("debug_cluster_path", path)
                s0, d0 = col.stat("sparse_clusters"), col.stat("dense_clusters")
                got = rs.cluster(col)
                ran = (col.stat("sparse_clusters") - s0, col.stat("dense_clusters") - d0)
                same_groups(got, col.cluster(rid))
                if len(rid) and col.kind != 0:   # (bool columns count two values in one kernel whatever the path)
                    assert ran == ((1, 0) if path == 1 else (0, 1))
            col.set_option("debug_cluster_path", 0)
        assert rs.stat("clusters") == 2 + 6
    assert sets[0].cluster(g)[3] == 2 and sets[0].cluster(age)[3] == 2
    # a field that was never built: no groups, every row missing
    raw_ix, raw_col = capi.GpuStringIndex(device=0), capi.GpuColumn("int64", device=0)
    same_groups(sets[0].cluster(raw_ix), raw_ix.cluster(some))
    same_groups(sets[0].cluster(raw_col), raw_col.cluster(some))
    assert sets[0].cluster(raw_ix)[3] == len(some) and sets[0].cluster(raw_col)[3] == len(some)
    with pytest.raises(TypeError):
        sets[0].cluster(None)
    for h in sets + [raw_ix, raw_col, dbl]:
        h.close()
