"""tests/column_referee.py pinned on the CPU: its numpy statement of a column's four arrays against a second one in plain Python
(sorted() over tuples, keys made with struct), and every named case checked for the edge it is named for."""
import struct

import numpy as np
import pytest

from tests import column_referee as R

TILE = R.TILE
APPEND = R.append_cases()
REMOVE = R.remove_cases()
BIG = 100000  # cases above this many rows are left to numpy alone (the plain-Python statement is slow, not different)


def py_key(kind, v):
    if kind == 1:
        return int(v) + (1 << 63)
    if kind == 2:
        d = float(v)
        if d == 0:
            d = 0.0  # -0.0 folds onto +0.0
        bits = struct.unpack("<Q", struct.pack("<d", d))[0]
        return (~bits) & ((1 << 64) - 1) if bits >> 63 else bits | (1 << 63)
    return 1 if v else 0


def py_arrays(kind, ids, values):
    rows = [(py_key(kind, v), int(i)) for i, v in zip(ids, values)]  # insertion order
    order = sorted(rows, key=lambda r: r[0]) if kind == 0 else sorted(rows)  # (sorted() is stable)
    id_sorted = sorted(i for _, i in rows)
    rank = {i: r for r, i in enumerate(id_sorted)}
    vpos = [0] * len(rows)
    for p, (_, i) in enumerate(order):
        vpos[rank[i]] = p
    return [k for k, _ in order], [i for _, i in order], id_sorted, vpos


def same(ref_arrays, py):
    return all(np.array_equal(np.asarray(a).astype(object), np.asarray(b, dtype=object)) for a, b in zip(ref_arrays, py))


def test_order_key_against_struct():
    dbl = np.array([0.0, -0.0, 1.5, -1.5, 5e-324, -5e-324, np.inf, -np.inf, 1e308, -1e308])
    assert [int(k) for k in R.order_key(2, dbl)] == [py_key(2, v) for v in dbl]
    assert R.order_key(2, [0.0])[0] == R.order_key(2, [-0.0])[0]
    assert list(np.argsort(R.order_key(2, dbl), kind="stable")) == list(np.argsort(dbl + 0.0, kind="stable"))
    i64 = np.array([0, -1, 1, -(1 << 63), (1 << 63) - 1], dtype=np.int64)
    assert [int(k) for k in R.order_key(1, i64)] == [py_key(1, v) for v in i64]
    assert list(R.order_key(0, [0, 1, 2, 255])) == [0, 1, 1, 1]
    with pytest.raises(ValueError):
        R.order_key(2, [1.0, float("nan")])


@pytest.mark.parametrize("name", [k for k, v in APPEND.items() if len(v[1]) + len(v[3]) <= BIG])
def test_append_against_plain_python(name):
    kinds, oi, ol, ni, nl = APPEND[name]
    for kind in kinds:
        c = R.RefColumn(kind)
        c.build(oi, R.values_of(kind, ol))
        assert same(c.arrays(), py_arrays(kind, oi, R.values_of(kind, ol)))
        assert c.append(ni, R.values_of(kind, nl)) == len(ni)
        allv = np.concatenate([R.values_of(kind, ol), R.values_of(kind, nl)])
        assert same(c.arrays(), py_arrays(kind, np.concatenate([oi, ni]), allv))
        assert c.n_false == (sum(1 for v in allv if not v) if kind == 0 else 0)


@pytest.mark.parametrize("name", [k for k, v in REMOVE.items() if len(v[1]) <= BIG])
def test_remove_against_plain_python(name):
    kinds, ids, lv, gone = REMOVE[name]
    for kind in kinds:
        vals = R.values_of(kind, lv)
        c = R.RefColumn(kind)
        c.build(ids, vals)
        removed, missing = c.remove(gone)
        held, gs = set(int(i) for i in ids), set(int(g) for g in gone)
        assert removed == len(held & gs) and missing == sum(1 for g in gone if int(g) not in held)
        keep = [j for j, i in enumerate(ids) if int(i) not in gs]
        assert same(c.arrays(), py_arrays(kind, ids[keep], vals[keep]))


def test_referee_refuses_duplicates():
    c = R.RefColumn(1)
    c.build([1, 2, 3], [5, 5, 5])
    with pytest.raises(ValueError, match="duplicate object id 2 in one column"):
        c.append([7, 2], [1, 1])
    with pytest.raises(ValueError, match="duplicate object id 9 in one column"):
        c.append([9, 9], [1, 1])
    assert list(c.ids) == [1, 2, 3]


def _new_positions(kind, oi, ol, ni, nl):
    c = R.RefColumn(kind)
    c.build(oi, R.values_of(kind, ol))
    concat = c.id_concat(ni)
    c.append(ni, R.values_of(kind, nl))
    keys_v, ids_v, _, _ = c.arrays()
    return np.flatnonzero(np.isin(ids_v, ni)), keys_v, ids_v, concat


def test_append_cases_reach_their_edges():
    for s in R.SIZES:
        assert len(APPEND[f"n_{s}"][1]) == s and len(APPEND[f"m_{s}"][3]) == s
    assert {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8193} == set(R.SIZES)
    assert len(APPEND["int64_257_tiles_plus_1"][1]) == 257 * TILE + 1
    for kind in (1, 2):
        n, m = len(APPEND["front"][1]), len(APPEND["front"][3])
        assert _new_positions(kind, *APPEND["front"][1:])[0].max() == m - 1
        assert _new_positions(kind, *APPEND["behind"][1:])[0].min() == n
        p = _new_positions(kind, *APPEND["one_gap_mid_tile"][1:])[0]
        assert p[-1] - p[0] == len(p) - 1 and p[0] // TILE == p[-1] // TILE and 0 < p[0] % TILE and p[-1] % TILE < TILE - 1
        assert list(_new_positions(kind, *APPEND["tile_first_and_last_slot"][1:])[0]) == [TILE, 2 * TILE - 1]
        p = _new_positions(kind, *APPEND["gap_larger_than_a_tile"][1:])[0]
        assert len(p) > TILE and p[0] == TILE and p[-1] >= 2 * TILE - 1   # output tile 1 holds new rows only
        p = _new_positions(kind, *APPEND["alternating"][1:])[0]
        assert np.array_equal(p, np.arange(len(p)) * 2 + 1)
        p, keys_v, ids_v, _ = _new_positions(kind, *APPEND["id_decides"][1:])
        old = np.flatnonzero(~np.isin(ids_v, APPEND["id_decides"][3]))
        q = old[(old > 0) & (old < len(ids_v) - 1)][0]   # an old row between a new id below and a new id above, same value
        assert keys_v[q - 1] == keys_v[q] == keys_v[q + 1] and ids_v[q - 1] == ids_v[q] - 3 and ids_v[q + 1] == ids_v[q] + 3
        assert {q - 1, q + 1} <= set(p)
    assert len(APPEND["m_above_n"][3]) > len(APPEND["m_above_n"][1]) > 0
    assert len(APPEND["empty_column"][1]) == 0
    _, oi, ol, ni, nl = APPEND["bool_ids_below"]
    p, keys_v, ids_v, concat = _new_positions(0, oi, ol, ni, nl)
    assert ni.max() < oi.min() and not concat
    for val in (0, 1):   # the new rows of a value lie behind every old row of that value
        pos_new = [q for q in p if keys_v[q] == val]
        pos_old = [q for q in np.flatnonzero(keys_v == val) if q not in set(p)]
        assert pos_new and pos_old and min(pos_new) > max(pos_old)
    assert _new_positions(1, *APPEND["ids_ascending_behind"][1:])[3] is True
    assert _new_positions(1, *APPEND["ids_interleaved"][1:])[3] is False
    assert _new_positions(1, *APPEND["ids_below"][1:])[3] is False
    oi = APPEND["ids_behind_unordered_build"][1]
    assert (np.diff(oi) < 0).any() and _new_positions(1, *APPEND["ids_behind_unordered_build"][1:])[3] is True
    oi = APPEND["ids_ascending_behind"][1]
    assert (np.diff(oi) > 0).all()
    # +0.0 against -0.0 (tests/test_gpu_column_maintain.py: the double-only case): equal keys, the id decides
    c = R.RefColumn(2)
    c.build([10, 20], [0.0, -0.0])
    c.append([15, 5], [-0.0, 0.0])
    assert list(c.arrays()[1]) == [5, 10, 15, 20] and len(set(c.arrays()[0])) == 1


def test_remove_cases_reach_their_edges():
    for s in R.SIZES:
        assert len(REMOVE[f"gone_{s}"][3]) == s and len(REMOVE[f"n_{s}"][1]) == s
    assert len(REMOVE["int64_257_tiles_plus_1"][1]) == 257 * TILE + 1

    def run(name, kind):
        _, ids, lv, gone = REMOVE[name]
        c = R.RefColumn(kind)
        c.build(ids, R.values_of(kind, lv))
        before = c.arrays()
        nf = c.n_false
        res = c.remove(gone)
        return before, nf, res, c

    for kind in (0, 1, 2):
        assert run("nothing_held", kind)[2] == (0, 3)
        before, _, res, c = run("everything", kind)
        assert res == (len(before[0]), 0) and len(c.ids) == 0
        assert len(run("all_but_one", kind)[3].ids) == 1
        assert run("twice_and_missing", kind)[2] == (300, 102)
        before, _, res, c = run("every_other", kind)
        assert res[0] * 2 == len(before[0])
    for kind in (1, 2):
        before, _, _, _ = run("first_and_last", kind)
        gone = REMOVE["first_and_last"][3]
        n = len(before[0])
        assert set(np.flatnonzero(np.isin(before[1], gone))) == {0, n - 1}     # value order
        assert set(np.flatnonzero(np.isin(before[2], gone))) == {0, n - 1}     # id order
        before, _, _, _ = run("whole_tile", kind)
        assert np.array_equal(np.flatnonzero(np.isin(before[1], REMOVE["whole_tile"][3])), np.arange(TILE, 2 * TILE))
    _, nf, _, c = run("bool_all_false", 0)
    assert nf > 0 and c.n_false == 0 and len(c.ids) > 0
