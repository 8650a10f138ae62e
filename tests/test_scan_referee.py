"""The scan referee (tests/scan_referee.py) pinned on the CPU: the operators and the fold against hand-written vectors, the numpy
scan against the fold, and every input builder against the edge it exists for — a case that stops covering its edge fails here,
without a GPU."""
import time

import numpy as np
import pytest

from tests import scan_referee as R

M = R.M64


def _l(a):
    return np.asarray(a).tolist()


def test_fold_hand_vectors():
    ex, inc, tot = R.fold(R.U64_ADD, [5, 1, M, 2])
    assert _l(ex) == [0, 5, 6, 5] and _l(inc) == [5, 6, 5, 7] and int(tot) == 7           # 6 + (2^64 - 1) wraps to 5
    ex, inc, tot = R.fold(R.U64_MAX, [3, 9, 2, 9, 10])
    assert _l(ex) == [0, 3, 9, 9, 9] and _l(inc) == [3, 9, 9, 9, 10] and int(tot) == 10
    ex, inc, tot = R.fold(R.U2_ADD, [[1, M], [2, 2], [3, 0]])
    assert _l(ex) == [[0, 0], [1, M], [3, 1]] and _l(inc) == [[1, M], [3, 1], [6, 1]] and _l(tot) == [6, 1]
    ex, inc, tot = R.fold(R.U2_SUMMAX, [[1, 4], [M, 2], [3, 7]])
    assert _l(ex) == [[0, 0], [1, 4], [0, 4]] and _l(inc) == [[1, 4], [0, 4], [3, 7]] and _l(tot) == [3, 7]
    # flag bytes: bit 1 = counted, bit 0 counted in the second half only beside bit 1; higher bits are ignored
    ex, inc, tot = R.fold(R.FLAGS_ADD, [0, 1, 2, 3, 0xFF, 0xFC])
    assert _l(inc) == [[0, 0], [0, 0], [1, 0], [2, 1], [3, 2], [3, 2]] and _l(ex) == [[0, 0]] + _l(inc)[:-1] and _l(tot) == [3, 2]


def test_docmax_hand_vectors():
    # the four-line definition: the right operand's document; the larger maximum inside a document, the right one's across documents
    assert R.combine(R.DOCMAX, (4, 9), (4, 3)) == (4, 9)
    assert R.combine(R.DOCMAX, (4, 3), (4, 9)) == (4, 9)
    assert R.combine(R.DOCMAX, (4, 9), (5, 3)) == (5, 3)
    assert R.combine(R.DOCMAX, (5, 3), (4, 9)) == (4, 9)
    ident = R.IDENTITY[R.DOCMAX]
    assert R.combine(R.DOCMAX, ident, (4, 9)) == (4, 9) and R.combine(R.DOCMAX, ident, (M, 0)) == (M, 0)   # a left identity ...
    assert R.combine(R.DOCMAX, (4, 9), ident) == ident                                                    # ... and only that
    # segments change at every position: nothing carries over
    every = [[0, 7], [1, 3], [2, 5], [3, 1]]
    ex, inc, tot = R.fold(R.DOCMAX, every)
    assert _l(inc) == every and _l(ex) == [[M, 0]] + every[:-1] and _l(tot) == [3, 1]
    # a single segment: a plain running maximum
    one = [[6, 2], [6, 9], [6, 4], [6, 9], [6, 11]]
    ex, inc, tot = R.fold(R.DOCMAX, one)
    assert _l(inc) == [[6, 2], [6, 9], [6, 9], [6, 9], [6, 11]] and _l(ex) == [[M, 0]] + _l(inc)[:-1] and _l(tot) == [6, 11]
    # document 0, a falling maximum, a later document with a smaller one
    mixed = [[0, 8], [0, 5], [0, 1], [3, 2], [3, 1]]
    assert _l(R.fold(R.DOCMAX, mixed)[1]) == [[0, 8], [0, 8], [0, 8], [3, 2], [3, 2]]
    for v in (every, one, mixed):
        for a, b in zip(R.fold(R.DOCMAX, v), R.scan(R.DOCMAX, v)):
            assert np.array_equal(a, b)


def test_empty_input():
    for kind in R.KINDS:
        for f in (R.fold, R.scan):
            ex, inc, tot = f(kind, np.zeros((0, 2) if kind in R.PAIR_KINDS and kind != R.FLAGS_ADD else 0, dtype=np.uint64))
            assert len(ex) == 0 and len(inc) == 0 and _l(tot) == (list(R.IDENTITY[kind]) if kind in R.PAIR_KINDS else R.IDENTITY[kind])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [1, 17, 1025, 4097])
def test_numpy_scan_equals_the_fold_on_every_input(kind, n):
    for name, items in R.scan_inputs(kind, n).items():
        for a, b in zip(R.fold(kind, items), R.scan(kind, items)):
            assert a.dtype == np.uint64 and np.array_equal(a, b), (R.KIND_NAMES[kind], n, name)


def test_docmax_referee_is_fast_enough_at_the_largest_size():
    n = R.SCAN_SIZES[-1]
    inputs = R.docmax_inputs(n)
    t0 = time.perf_counter()
    for items in inputs.values():
        R.scan(R.DOCMAX, items)
    per_input = (time.perf_counter() - t0) / len(inputs)
    assert per_input < 2.0, per_input


def test_docmax_inputs_keep_documents_adjacent_and_cover_their_edges():
    for n in (33, 4097, 3 * 4096 + 1):
        inputs = R.docmax_inputs(n)
        for name, a in inputs.items():
            doc = a[:, 0]
            starts = np.flatnonzero(np.r_[True, doc[1:] != doc[:-1]])
            assert len(np.unique(doc)) == len(starts), (n, name)     # every document is one run: the operator is associative here
            assert name == "identity" or not np.any(doc == np.uint64(M)), (n, name)
        assert len(np.unique(inputs["one_document"][:, 0])) == 1 and len(np.unique(inputs["every_item_new"][:, 0])) == n
        assert np.all(np.diff(inputs["decreasing"][:, 1].astype(np.int64)) < 0)
        for off, name in ((-1, "starts_before_boundary"), (0, "starts_at_boundary"), (1, "starts_after_boundary")):
            doc = inputs[name][:, 0]
            assert doc[0] == 0                                          # a document id equal to 0
            starts = np.flatnonzero(doc[1:] != doc[:-1]) + 1
            want = [b + off for unit in (R.IPT, R.WAVE, R.TILE) for b in range(unit, n + 1, unit) if 0 < b + off < n]
            assert set(want) <= set(starts.tolist()) and all((s - off) % R.IPT == 0 for s in starts), (n, name)
    a = R.docmax_inputs(3 * 4096 + 1)["max_in_earlier_tile"]
    long_doc = np.flatnonzero(a[:, 0] == a[5, 0])
    assert int(np.argmax(a[:, 1])) == 5 and 5 // R.TILE < long_doc[-1] // R.TILE and long_doc[0] <= 5


def test_max_inputs_put_the_maximum_where_they_say():
    u = R.u64_inputs(R.U64_MAX, 3 * 4096 + 1)
    assert np.argmax(u["max_first"]) == 0 and np.argmax(u["max_last"]) == 3 * 4096
    assert np.argmax(u["max_lane63"]) == 1023 and (1023 // R.IPT) % 64 == 63
    assert np.argmax(u["max_tile_end"]) == 4095 and np.argmax(u["max_second_tile_end"]) == 8191
    s = R.u2_inputs(R.U2_SUMMAX, 3 * 4096 + 1)
    assert np.argmax(s["max_first_tile"][:, 1]) == 2048 and np.argmax(s["max_first"][:, 1]) == 0
    w = R.u64_inputs(R.U64_ADD, 17)["wrap"]
    assert int(w[0]) + int(w[1]) + int(w[2]) > M                  # the sums do wrap


def test_flag_inputs_cover_every_pair_across_the_load_boundary():
    for n in (4096, 4097):
        f = R.flag_inputs(n)
        assert n % 16 == 0 or n % 16 == 1
        for name in ("across_loads",):
            a = f[name]
            across = {(int(a[i - 1]), int(a[i])) for i in range(16, n, 16)}       # last byte of one load, first of the next
            inside = {(int(a[i - 1]), int(a[i])) for i in range(1, n) if i % 16}
            assert across == {(x, y) for x in range(4) for y in range(4)}, (name, n)
            assert inside == across, (name, n)


def test_stable_rank_referee_and_patterns():
    before, base, total = R.stable_ranks([0, 2, 0, 1, 1, 0])
    assert _l(before) == [0, 0, 1, 1, 2, 3] and _l(base) == [0] and total == 3
    n = 2 * 4096 + 1
    p = R.rank_patterns(n)
    before, base, total = R.stable_ranks(p["all"])
    assert _l(before[:3]) == [0, 1, 2] and _l(base) == [0, 4096, 8192] and total == n
    assert _l(np.flatnonzero(p["lane63"])[:3]) == [63, 127, 191] and _l(np.flatnonzero(p["wave3"])[:2]) == [192, 193]
    assert _l(np.flatnonzero(p["round15"])[[0, -1]]) == [15 * 256, 4096 + 4095] and _l(np.flatnonzero(p["round0"])[[0, 256]]) == [0, 4096]
    assert set(((np.flatnonzero(p["odd_rounds"]) % 4096) // 256).tolist()) == set(range(1, 16, 2))
    for at in R.SINGLE_SLOTS + (n - 1,):
        assert _l(np.flatnonzero(p[f"single_{at}"])) == [at]
    assert 0 < p["random_1"].astype(bool).mean() < 0.03 and p["random_99"].astype(bool).mean() > 0.97
    assert set(R.rank_patterns(1)) >= {"none", "all", "single_0"}
