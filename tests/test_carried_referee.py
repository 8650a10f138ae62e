"""The referee of the in-place carried round (tests/carried_referee.py) against itself: its two statements of the rule agree on
every case, every case reaches the edge it is named for, and the in-place step followed by the carried round over what is
left equals the carried round over everything.  CPU only."""
import re

import numpy as np
import pytest

from tests import carried_referee as R

CASES = R.cases()


@pytest.fixture(scope="module")
def results():
    return {name: R.inplace_ints(*c) for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_forms_agree(name, results):
    e, f, partials, met, moved, _ = results[name]
    e2, f2, partials2, met2, moved2 = R.inplace_numpy(*CASES[name])
    assert np.array_equal(np.array(e, dtype=np.uint64), e2)
    assert np.array_equal(np.array(f, dtype=np.uint8), f2)
    assert np.array_equal(np.array(partials, dtype=np.uint64).reshape(-1, 2), partials2)
    assert (met, moved) == (met2, moved2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_in_place_then_the_round_over_the_rest_is_the_round_over_everything(name, results):
    e0, f0, x = CASES[name]
    e, f = results[name][:2]
    ea, fa = R.carried_round(e, f, x)
    eb, fb = R.carried_round(e0, f0, x)
    assert ea == eb
    open0 = [bool(v & 2) for v in f0]
    assert [v & 3 for v, o in zip(fa, open0) if o] == [v & 3 for v, o in zip(fb, open0) if o]
    # slots that were not open are nobody's: entry and whole flag byte as they came
    assert all(f[i] == int(f0[i]) and e[i] == int(e0[i]) for i, o in enumerate(open0) if not o)
    # the entries are a permutation, and the carried bits went with them
    bits0 = {int(v): int(b) >> 2 for v, b in zip(e0, f0)}
    assert sorted(e) == sorted(int(v) for v in e0)
    assert all(f[i] >> 2 == bits0[e[i]] for i in range(len(e)))


def test_every_case_reaches_its_edge(results):
    T = R.TILE
    seen = set()
    for name, (e, f, partials, met, moved, info) in results.items():
        e0, f0, x = CASES[name]
        n = len(e0)
        f0 = np.asarray(f0)
        f = np.array(f, dtype=np.uint8)
        m = re.match(r"([a-z_]+?)_?(\d+)?(?:_([a-z]+))?$", name)
        if name.startswith("len_"):
            assert n == int(name[4:]) and len(partials) == (n + T - 1) // T
            assert info["owned"] > 0 and (n < 3 * T or moved > 0)
        elif name.startswith("size_"):
            size, kind = int(m.group(2)), m.group(3)
            opened = np.flatnonzero(f0 & 2)
            if size > R.GROUP_MAX:
                assert info["long"] == 4 and info["owned"] == 0 and moved == 0 and np.array_equal(f, f0)
            else:
                assert info["owned"] == 4 and info["sizes"] == {size} and info["long"] == 0
                if kind == "equal":       # nothing moves and the groups stay open
                    assert moved == 0 and np.array_equal(f, f0) and info["settled"] == 0
                elif kind == "distinct":  # fully settled: bit 1 cleared everywhere
                    assert info["kept_open"] == 0 and not np.any(f[opened] & 2) and np.all(f[opened] & 1)
                elif kind == "descending" and size <= 1 << x:  # every slot changes (the middle of an odd group but for its flag)
                    assert moved == 4 * (size - size % 2) and np.all(f[opened] != f0[opened])
                elif kind == "two":       # stability: both values keep their order, and they part into two groups
                    z, t = size // 2, size - size // 2   # (members with the smaller and with the greater value)
                    assert moved > 0 and info["kept_open"] == 4 * ((z if z > 1 else 0) + (t if t > 1 else 0))
            seen.add(("size", size))
        elif name.startswith("x_"):
            assert x == int(name[2:]) and moved > 0 and info["settled"] > 0
            if x < 6:                     # bits above the key are live and travel
                assert np.any((f0 >> (2 + x)) != 0)
        elif name == "head_on_tile_last_slot":
            assert f0[T - 1] & 3 == 3 and info["crossing"] == 1 and info["headless"] == 2
            assert f0[2 * T - 1] & 3 == 2 and f0[2 * T] & 3 == 3 and info["owned"] == 2
        elif name == "ends_on_tile_last_slot":
            assert f0[2 * T - 1] & 3 == 2 and f0[2 * T] & 3 == 1 and f0[n - 1] & 3 == 2 and info["owned"] == 2 and info["crossing"] == 0
        elif name == "group_spans_a_tile":
            assert info["crossing"] == 1 and info["headless"] == T + 20 and info["owned"] == 1 and info["long"] == 0
        elif name == "headless_leading_members":
            assert info["headless"] == 7 and info["owned"] == 2 and info["crossing"] == 1 and f0[0] & 3 == 2 and f0[T] & 3 == 2
        elif name.startswith("trip_boundary_"):
            o = int(name[len("trip_boundary_"):])
            pos = R.list_positions(f0)
            heads = [s for s in pos if f0[s] & 1]
            cut = [h for h in heads if pos[h] == 64 - o]
            assert len(cut) == 1
            members = [s for s in pos if s >= cut[0] and pos[s] < pos[cut[0]] + min(64, o + 2)]
            assert pos[members[0]] < 64 <= pos[members[-1]] and info["long"] == 0 and moved > 0
            seen.add(("trip", o))
        elif name.startswith("window_"):
            total = int(name.split("_")[1])
            assert partials[0] == (0, 0) and len(R.list_positions(f0, 1)) == total == met and info["long"] == 0 and moved > total // 4
            seen.add(("window", total))
        elif name == "long_between_short":
            assert info["long"] == 2 and info["owned"] == 4 and 64 in info["sizes"]
        elif name == "closed_groups_live_bits":
            assert met == 0 and moved == 0 and np.array_equal(f, f0) and np.any((f0 & 3) == 0) and np.any(f0[(f0 & 3) == 0] >> 2)
            assert all(p == (0, 0) for p in partials)
        elif name == "tiles_with_nothing_open":
            assert partials[0] == (0, 0) and partials[2] == (0, 0) and met == 2 and moved == 2
        elif name == "list_fills_a_tile":
            assert np.all(f0[T:2 * T] & 2) and info["crossing"] == 0 and info["owned"] > 400
        elif name == "one_group_fills_a_tile":
            assert info["long"] == 1 and moved == 0 and partials[0] == (T, 1)
        else:
            raise AssertionError(f"case {name} names no edge")
    assert {("size", s) for s in (2, 3, 63, 64, 65)} <= seen and {("trip", o) for o in range(1, 64)} <= seen
    W = R.LIST_WINDOW
    assert {("window", t) for t in (W - 1, W, W + 1, W + 26, W + 63, W + 64, W + 65, 2 * W + 30, 3 * W - 70)} <= seen
    need = {1, 2, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1, (R.TILES_PER_WAVE + 1) * T - 5, (R.TILES_PER_WORKGROUP + 1) * T - 7}
    assert need <= {len(c[0]) for c in CASES.values()}
    # 40-bit entries with non-zero high bytes, lengths that are no multiple of 16
    assert all(np.all(np.asarray(c[0]) >> np.uint64(32)) for c in CASES.values())
    assert any(len(c[0]) % 16 for c in CASES.values())
