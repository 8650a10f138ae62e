"""The last pass over the cells of the top-digit-first segmented sort (radix_pass.h: SegFinalCellArgs) at the edges of what is its
own: head and tail from the neighbouring 32-bit keys alone, one read of the aux byte for the flag byte and the entry, 16-byte edge
records (seg_cell_edge.h) and their edge fix (radix_sort.h: rs_seg_edge_fix_cell_kernel).  Through cdb_debug_segsort with the
production functions, against tests/segsort_referee.py with exact integer equality of entries, flag bytes and cell table.

The last pass sorts a cell on bits 24..31 of its 32-bit keys; its tiles are the cell's records in the order of the three passes in
front of it (stable by the low 24 bits), 16384 to a tile.  A (tile, digit) run leaves one edge record; equal keys sit next to each
other in that order, so a tied group crosses from one run to the next exactly where it straddles a tile end.  Every case below
states in `reaches` the edge it is named for, from that order, before anything runs on the device."""
import numpy as np
import pytest

from tests import segsort_referee as R

pytestmark = pytest.mark.gpu

TILE = R.TILE
U = np.uint64


def last_pass_view(c, cell):
    """(k32, original index) of the records of cell number `cell` in the order the last pass reads them"""
    seen = 0
    for b in range(len(c.bucket_begin) - 1):
        lo, hi = int(c.bucket_begin[b]), int(c.bucket_begin[b + 1])
        tops = c.key[lo:hi] >> U(32)
        for top in np.unique(tops):
            if seen == cell:
                idx = lo + np.flatnonzero(tops == top)      # (the top pass is stable: bucket order)
                k32 = c.key[idx] & U(0xFFFFFFFF)
                order = np.argsort(k32 & U(0xFFFFFF), kind="stable")
                return k32[order], idx[order]
            seen += 1
    raise IndexError(cell)


def runs(k32):
    """{(tile, digit): (first key, last key, count)} of a last-pass view"""
    out = {}
    for t in range(0, len(k32), TILE):
        part = k32[t:t + TILE]
        for d in np.unique(part >> U(24)):
            ks = np.sort(part[(part >> U(24)) == d])
            out[(t // TILE, int(d))] = (int(ks[0]), int(ks[-1]), len(ks))
    return out


def _distinct(rng, n, lo24, hi24, digits):
    """n keys with distinct low 24 bits in [lo24, hi24) and a last-pass digit drawn from `digits`"""
    low = rng.permutation(np.unique(rng.integers(lo24, hi24, size=2 * n + 64, dtype=np.uint64)))[:n]
    assert len(low) == n
    return (rng.choice(np.asarray(digits, dtype=np.uint64), size=n) << U(24)) | low


def _flags_at(c, keyval):
    """the referee's flag bytes (without the carried bits) of the slots that hold 40-bit key `keyval`, in output order"""
    e, f = R.referee_numpy(*c.args())
    bucket = np.repeat(np.arange(len(c.bucket_begin) - 1), np.diff(c.bucket_begin.astype(np.int64)))
    k = c.key[np.lexsort((np.arange(len(c.key)), c.key, bucket))]
    return [int(x) & 3 for x in f[k == U(keyval)]]


def build_cases(ehb, carry):
    rng = np.random.default_rng(4242)
    out = {}

    def add(name, buckets, reaches, edit=None):
        c = R.Case(name, buckets, ehb=ehb, carry=carry, seed=len(out))
        if edit:
            edit(c)
        assert reaches(c), f"case {name} does not reach the edge it is named for"
        out[name] = c

    # ---- one run of a whole tile (cnt = 16384 in one edge record), tied across the edge with the tile behind it
    D = 0x5A
    tied = (D << 24) | 0xFFFFF1                                              # (odd: the group stays open)
    one_digit = np.concatenate([_distinct(rng, TILE - 84, 0, 0xFFFFF0, [D]), np.full(184, tied, dtype=np.uint64)])

    def full_run(c):
        k, _ = last_pass_view(c, 0)
        r = runs(k)
        return set(r) == {(0, D), (1, D)} and r[(0, D)][2] == TILE and r[(0, D)][1] == tied == r[(1, D)][0] == r[(1, D)][1] \
            and _flags_at(c, (7 << 32) | tied) == [3] + [2] * 183
    add("run_of_a_whole_tile_tied_with_the_next", [[(7, one_digit)]], full_run)

    # ---- a pair tied across a tile end and nothing else: joined by the edge fix alone; bit 0 clear and set
    def straddle(pair, n_behind):
        front = _distinct(rng, TILE - 1, 0, 0x800000, [0, 7, 255])
        behind = _distinct(rng, n_behind, 0x800002, 0x1000000, [0, 7, 255])
        return np.concatenate([front, np.full(2, pair, dtype=np.uint64), behind])
    even, odd = (7 << 24) | 0x800000, (7 << 24) | 0x800001

    def pair_joined(c):
        ok = True
        for cell, (top, pair) in enumerate(((1, even), (2, odd))):
            k, _ = last_pass_view(c, cell)
            r = runs(k)
            ok = ok and k[TILE - 1] == pair == k[TILE] and r[(0, 7)][1] == pair == r[(1, 7)][0] and r[(0, 7)][2] > 1 and r[(1, 7)][2] > 1 \
                and _flags_at(c, (top << 32) | pair) == ([1, 0] if pair == even else [3, 2])
        return ok
    add("pair_across_a_tile_end_bit0_clear_and_set", [[(1, straddle(even, TILE - 37)), (2, straddle(odd, 900))]], pair_joined)

    # ---- keys 0 and 0xFFFFFFFF as first and last of their runs, the all-ones keys beside the padding of a ragged tile
    zeros, ones = np.zeros(300, dtype=np.uint64), np.full(300, 0xFFFFFFFF, dtype=np.uint64)
    ragged = np.concatenate([zeros, ones, _distinct(rng, TILE - 100, 1, 0xFFFFFF, [0, 3, 255])])

    def extremes(c):
        k, _ = last_pass_view(c, 0)
        r = runs(k)
        return len(k) == TILE + 500 and r[(0, 0)][0] == 0 and r[(1, 255)][1] == 0xFFFFFFFF and (0, 255) in r and (1, 0) in r \
            and r[(1, 0)][0] != 0 and r[(0, 255)][1] != 0xFFFFFFFF and _flags_at(c, 9 << 32) == [1] + [0] * 299 \
            and _flags_at(c, (9 << 32) | 0xFFFFFFFF) == [3] + [2] * 299
    add("all_zero_and_all_ones_keys_beside_the_padding", [[(9, ragged)]], extremes)

    # ---- a tied pair across a tile end whose aux bytes differ in every bit: the byte is no part of the key, and each entry keeps its own
    def differ(c):
        i = np.flatnonzero(c.key == U((3 << 32) | odd))
        assert len(i) == 2
        c.entry[i[0]], c.entry[i[1]] = U(5), U(((1 << ehb) - 1) << 32 | 6)
        if carry:
            c.carried[i[0]], c.carried[i[1]] = 0b010101, 0b101010

    def aux_differs(c):
        k, idx = last_pass_view(c, 0)
        a, b = idx[TILE - 1], idx[TILE]
        hi = lambda i: int(c.entry[i]) >> 32 | int(c.carried[i]) << ehb
        return k[TILE - 1] == odd == k[TILE] and hi(a) ^ hi(b) == (1 << (ehb + carry)) - 1 and _flags_at(c, (3 << 32) | odd) == [3, 2]
    add("tied_pair_with_different_aux_bytes", [[(3, straddle(odd, 333))]], aux_differs, edit=differ)

    # ---- a digit absent from several consecutive tiles (the edge fix searches for the run in front), and a digit whose first run
    #      in the cell is not in the cell's first tile
    gap = np.concatenate([_distinct(rng, 500, 0, 0x010000, [9]), _distinct(rng, 500, 0xFF0000, 0x1000000, [9]),
                          _distinct(rng, 200, 0xFE0000, 0xFF0000, [5]), _distinct(rng, 5 * TILE - 1200 - 11, 0x010000, 0xFE0000, [1, 2])])

    def searched(c):
        k, _ = last_pass_view(c, 0)
        r = runs(k)
        nine = sorted(t for t, d in r if d == 9)
        five = sorted(t for t, d in r if d == 5)
        return nine == [0, 4] and five == [4] and all((t, 1) in r and (t, 2) in r for t in range(5))
    add("digit_absent_from_three_tiles_and_a_late_first_run", [[(0x44, gap)], [(0x44, _distinct(rng, 50, 0, 1 << 24, [9, 5]))]], searched)
    return out


FORMS = {"carried_6": (2, 6), "carried_0": (2, 0)}   # (entry bits 32.. , carried bits) of the aux byte
NAMES = ["all_zero_and_all_ones_keys_beside_the_padding", "digit_absent_from_three_tiles_and_a_late_first_run",
         "pair_across_a_tile_end_bit0_clear_and_set", "run_of_a_whole_tile_tied_with_the_next", "tied_pair_with_different_aux_bytes"]


@pytest.fixture(scope="module")
def cases():
    out = {f: build_cases(*ec) for f, ec in FORMS.items()}   # (built, and every `reaches` checked, when the first test runs: not at collection)
    assert all(sorted(cs) == NAMES for cs in out.values())
    return out


@pytest.fixture(scope="module")
def capi():
    from coffeedb_amd import capi
    capi.load_library()
    return capi


@pytest.fixture(scope="module")
def expected(cases):
    return {(f, n): R.referee_numpy(*c.args()) for f, cs in cases.items() for n, c in cs.items()}   # (once, shared, never written to)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "plain"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", NAMES)
def test_last_pass_over_cells(capi, cases, expected, name, form, packed):
    c = cases[form][name]
    k32, v32, w16 = R.split(True, c.key, c.entry, c.carried, c.ehb)
    e, f, cells, ok = capi.debug_segsort(capi.SEGSORT_TOP_FIRST, c.bucket_begin, k32, v32, w16, c.ehb, c.carry, packed=packed)
    re_, rf = expected[(form, name)]
    assert ok, "a guard around a device array was written"
    assert np.array_equal(e, re_), np.flatnonzero(e != re_)[:8]
    assert np.array_equal(f, rf), (np.flatnonzero(f != rf)[:8], f[f != rf][:8], rf[f != rf][:8])
    assert np.array_equal(cells, R.cells(c.bucket_begin, c.key))
