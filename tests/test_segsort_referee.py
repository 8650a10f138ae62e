"""Pins tests/segsort_referee.py on the CPU: its two statements (Python integers, numpy) agree on every case, every case reaches the
edge it is named for (cases() asserts that while it builds them), and the two record splits carry the same records."""
import numpy as np
import pytest

from tests import segsort_referee as R

CASES = R.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_statements_agree(name):
    c = CASES[name]
    e, f = R.referee(*c.args())
    en, fn = R.referee_numpy(*c.args())
    assert np.array_equal(np.array(e, dtype=np.uint64), en) and np.array_equal(np.array(f, dtype=np.uint8), fn)
    assert sorted(e) == sorted(int(x) for x in c.entry)
    assert all((x >> 2) < (1 << c.carry) for x in f)


def test_the_issue_s_edges_are_all_there():
    sizes = list(CASES["cell_sizes_at_the_tile"].cell_sizes())
    assert sizes == [1, 2, R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE + 1]
    assert len(R.cells(*CASES["cell_table_of_258_cells"].args()[:2])) == 258
    assert {(c.ehb, c.carry) for c in CASES.values()} >= {(1, 5), (3, 5), (8, 0), (2, 6), (1, 0)}
    assert max(len(c.key) for c in CASES.values()) <= 1 << 18


@pytest.mark.parametrize("name", ["one_bucket", "tied_groups_meet_at_a_cell_border", "entry_high_bits_8_carried_0"])
def test_splits_hold_the_same_records(name):
    c = CASES[name]
    k5, v5, w5 = R.split(False, c.key, c.entry, c.carried, c.ehb)
    kt, vt, wt = R.split(True, c.key, c.entry, c.carried, c.ehb)
    key5 = k5.astype(np.uint64) << np.uint64(8) | (w5 & np.uint16(0xFF)).astype(np.uint64)
    keyt = (wt & np.uint16(0xFF)).astype(np.uint64) << np.uint64(32) | kt.astype(np.uint64)
    assert np.array_equal(key5, c.key) and np.array_equal(keyt, c.key) and np.array_equal(v5, vt)
    assert np.array_equal(w5 >> np.uint16(8), wt >> np.uint16(8))
    hi = (w5 >> np.uint16(8)).astype(np.uint64)
    assert np.array_equal((hi & np.uint64((1 << c.ehb) - 1)) << np.uint64(32) | v5.astype(np.uint64), c.entry)
    assert np.array_equal((hi >> np.uint64(c.ehb)).astype(np.uint8), c.carried)


def test_flags_of_a_hand_made_bucket():
    # bucket 0: keys 5 5 4(even) 4 9 -> sorted 4 4 5 5 9: the even pair is closed (ends inside the document), the odd pair open
    bb, key = [0, 5, 6], [5, 5, 4, 4, 9, 5]
    e, f = R.referee(bb, key, [10, 11, 12, 13, 14, 15], [0, 1, 2, 3, 0, 1])
    assert e == [12, 13, 10, 11, 14, 15]
    assert f == [1 | 2 << 2, 0 | 3 << 2, 1 | 2, 2 | 1 << 2, 1, 1 | 1 << 2]
