"""The device-wide scan (scan.h) and the stable tile ranks (stable_tiles.h) on their own, at the edges of their items, threads,
waves, tiles, sweeps and levels, called as the library calls them (cdb_debug_scan / cdb_debug_scan_partials /
cdb_debug_stable_ranks, debug_scan.hip) and compared with the referee of tests/scan_referee.py.

Every comparison is integer equality."""
import numpy as np
import pytest

from tests import scan_referee as R

pytestmark = pytest.mark.gpu

E_INVALID = 1
TWO_SIDED = (R.U64_ADD, R.U64_MAX, R.U2_ADD, R.U2_SUMMAX, R.FLAGS_ADD)


def _kind_id(kind):
    return R.KIND_NAMES[kind]


def _wrong(got, want):
    """the items (rows) that differ"""
    m = got != want
    return np.flatnonzero(m.any(axis=1) if m.ndim > 1 else m)


@pytest.mark.parametrize("n", R.SCAN_SIZES)
@pytest.mark.parametrize("kind", R.KINDS, ids=_kind_id)
def test_scan_at_item_thread_wave_and_tile_edges(kind, n):
    """n around one item, one thread (16 items), one wave (1024), one tile (4096), several tiles, and 257 tiles + 1 where the sweep
    over the tile partials has a ragged thread of its own.

    out_total is NOT compared for DocMax: its identity {~0, 0} is a left identity only, the kernels pad the last tile with it on the
    right, and production discards the value scan_totals returns for it.  Every other kind's total is asserted."""
    from coffeedb_amd import capi
    for name, items in R.scan_inputs(kind, n).items():
        want_ex, want_inc, want_total = R.scan(kind, items)
        ex, inc, total = capi.debug_scan(kind, items)
        what = (R.KIND_NAMES[kind], n, name)
        assert ex.shape == want_ex.shape and inc.shape == want_inc.shape, what
        bad = _wrong(inc, want_inc)
        assert len(bad) == 0, ("inclusive", what, "first wrong item", int(bad[0]), inc[bad[0]].tolist(), want_inc[bad[0]].tolist())
        bad = _wrong(ex, want_ex)
        assert len(bad) == 0, ("exclusive", what, "first wrong item", int(bad[0]), ex[bad[0]].tolist(), want_ex[bad[0]].tolist())
        if kind in TWO_SIDED:
            assert np.array_equal(total, want_total), ("total", what, total.tolist(), want_total.tolist())


@pytest.mark.parametrize("nb", R.PARTIALS_SIZES)
@pytest.mark.parametrize("kind", R.PARTIALS_KINDS, ids=_kind_id)
def test_partials_scan_at_sweep_and_level_edges(kind, nb):
    """scan_partials_inplace in its three regimes — one sweep (up to 16 384 partials), several sweeps with a carry (up to 2^16), a
    second level behind the first (beyond) — in a block of exactly the elements scan_totals reserves, with poison behind it."""
    from coffeedb_amd import capi
    for name, sums in R.partials_inputs(kind, nb).items():
        want_ex, _, want_total = R.scan(kind, sums)
        ex, total, guard_ok = capi.debug_scan_partials(kind, sums, guard_words=64)
        what = (R.KIND_NAMES[kind], nb, name)
        assert guard_ok, ("the scan wrote behind its block", what)
        bad = _wrong(ex, want_ex)
        assert len(bad) == 0, ("prefix", what, "first wrong slot", int(bad[0]), ex[bad[0]].tolist(), want_ex[bad[0]].tolist())
        if kind in TWO_SIDED:      # (slot nb of the one-sided DocMax is not part of the contract: see the scan test)
            assert np.array_equal(total, want_total), ("grand total in slot nb", what, total.tolist(), want_total.tolist())


def _check_ranks(flags, what):
    from coffeedb_amd import capi
    want_before, want_base, want_total = R.stable_ranks(flags)
    before, base, total = capi.debug_stable_ranks(flags)
    assert total == want_total == int(np.count_nonzero(flags)), ("total", what, total, want_total)
    assert np.array_equal(base, want_base), ("tile_base", what)
    bad = np.flatnonzero(before != want_before)
    assert len(bad) == 0, ("before", what, "first wrong slot", int(bad[0]), int(before[bad[0]]), int(want_before[bad[0]]))


@pytest.mark.parametrize("n", R.RANK_SIZES)
def test_stable_ranks_for_flags_on_chosen_lanes_waves_rounds_and_tiles(n):
    """The rank of every slot, flagged or not, for flags on lane 0 / lane 63 of every wave, one wave, one round, the odd rounds (one
    half of TileRanker's two-half exchange), single slots, and random densities.

    What this cannot show: that the exchange NEEDS its two halves.  With one barrier per round, a single buffer is wrong only if a
    wave writes its count of round k + 1 before another wave has read those of round k — the reader's LDS loads directly follow the
    barrier, the writer's store follows its next flag load — and a library built that way passed every case here on an MI355X.  The
    values, the barrier and the round order are what these cases pin."""
    for name, flags in R.rank_patterns(n).items():
        _check_ranks(flags, (n, name))


def test_stable_ranks_where_the_tile_counts_cross_a_scan_tile():
    """4097 tiles + 3 slots: the scan over the tile counts itself has a second tile (16 MiB of flags, 134 MB of ranks; one case)"""
    n = R.RANK_BIG
    i = np.arange(n, dtype=np.int64)
    flags = (((i * 2654435761) >> 7) % 3 != 0).astype(np.uint8)      # about two in three, no period of the tile's
    flags[-3:] = (1, 0, 1)
    _check_ranks(flags, (n, "two_in_three"))


def test_stable_ranks_refuse_an_empty_array():
    from coffeedb_amd import capi
    with pytest.raises(capi.ScanError) as e:
        capi.debug_stable_ranks(np.zeros(0, dtype=np.uint8))
    assert e.value.status == E_INVALID
