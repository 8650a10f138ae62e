"""The segmented sort of bucket records in its two forms — five passes over 10-byte records, and top key digit first with 9-byte
records inside (bucket, top byte) cells (radix_sort.h: radix_sort_top_first) — run through cdb_debug_segsort (debug_segsort.hip)
with the production functions, against the referee of tests/segsort_referee.py with exact integer equality: entries (written
packed and plain), flag bytes, the cell table, and the guards around every device array."""
import numpy as np
import pytest

from tests import segsort_referee as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


@pytest.fixture(scope="module")
def capi():
    from coffeedb_amd import capi
    capi.load_library()
    return capi


@pytest.fixture(scope="module")
def expected():
    return {name: R.referee_numpy(*c.args()) for name, c in CASES.items()}   # (computed once, shared, never written to)


def _run(capi, c, form, packed):
    k32, v32, w16 = R.split(form == capi.SEGSORT_TOP_FIRST, c.key, c.entry, c.carried, c.ehb)
    return capi.debug_segsort(form, c.bucket_begin, k32, v32, w16, c.ehb, c.carry, packed=packed)


def _check(capi, expected, name, form, packed):
    c = CASES[name]
    e, f, cells, ok = _run(capi, c, form, packed)
    re_, rf = expected[name]
    assert ok, "a guard around a device array was written"
    assert np.array_equal(e, re_), np.flatnonzero(e != re_)[:8]
    assert np.array_equal(f, rf), (np.flatnonzero(f != rf)[:8], f[f != rf][:8], rf[f != rf][:8])
    if form == capi.SEGSORT_TOP_FIRST:
        assert np.array_equal(cells, R.cells(c.bucket_begin, c.key))
    else:
        assert len(cells) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_top_first_packed(capi, expected, name):
    _check(capi, expected, name, capi.SEGSORT_TOP_FIRST, True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_five_pass_packed(capi, expected, name):
    _check(capi, expected, name, capi.SEGSORT_FIVE_PASS, True)


PLAIN = ["cell_sizes_at_the_tile", "tied_groups_meet_at_a_cell_border", "entry_high_bits_8_carried_0", "entry_high_bits_2_carried_6",
         "cell_table_of_258_cells"]


@pytest.mark.parametrize("name", PLAIN)
def test_plain_entries(capi, expected, name):
    _check(capi, expected, name, capi.SEGSORT_TOP_FIRST, False)
    _check(capi, expected, name, capi.SEGSORT_FIVE_PASS, False)


def test_hook_refuses_what_the_build_never_passes(capi):
    c = CASES["one_bucket"]
    k32, v32, w16 = R.split(True, c.key, c.entry, c.carried, c.ehb)
    for bad in (dict(ehb=9, carry=0), dict(ehb=3, carry=6), dict(ehb=0, carry=2)):   # (the aux words hold 3 + 5 bits)
        with pytest.raises(capi.SegsortError) as err:
            capi.debug_segsort(capi.SEGSORT_TOP_FIRST, c.bucket_begin, k32, v32, w16, bad["ehb"], bad["carry"])
        assert err.value.status == 1
    with pytest.raises(capi.SegsortError):
        capi.debug_segsort(capi.SEGSORT_TOP_FIRST, [0, len(k32), len(k32)], k32, v32, w16, c.ehb, c.carry)   # the last bucket is empty
