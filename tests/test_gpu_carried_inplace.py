"""The in-place carried round (carried_inplace.h: sa_carried_inplace_kernel): the kernel, launched the way refine_groups launches
it (cdb_debug_carried_inplace, debug_carried.hip), against the referee of tests/carried_referee.py with exact integer equality —
entries, flag bytes, tile sums, the entries met and moved, and the guards around every device array — and whole builds with the
sweep on, off and without carried bits against the CPU oracle and each other."""
import numpy as np
import pytest

from coffeedb_amd import workloads as W
from tests import carried_referee as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
VL = dict(force_big_path=1, vl_keys=40)


@pytest.fixture(scope="module")
def capi():
    from coffeedb_amd import capi
    capi.load_library()
    return capi


def _check(capi, name, form, mask=None):
    e0, f0, x = CASES[name]
    if mask is not None:
        e0 = e0 & np.uint64(mask)
        assert len(np.unique(e0)) == len(e0)
    e, f, partials, met, moved, ok = capi.debug_carried_inplace(e0, f0, x, form=form)
    re_, rf, rp, rmet, rmoved = R.inplace_numpy(e0, f0, x)
    assert ok, "a guard around a device array was written"
    assert np.array_equal(f, rf), np.flatnonzero(f != rf)[:8]
    assert np.array_equal(e, re_), np.flatnonzero(e != re_)[:8]
    assert np.array_equal(partials, rp), np.flatnonzero(partials != rp)[:8]
    assert (met, moved) == (rmet, rmoved)


@pytest.mark.parametrize("name", sorted(CASES))
def test_packed_entries(capi, name):
    _check(capi, name, capi.CARRIED_PACKED40)


PLAIN = ["len_1", "len_17", "len_4097", f"len_{(R.TILES_PER_WORKGROUP + 1) * R.TILE - 7}", "size_3_descending", "size_64_random",
         "size_65_two", "x_1", "x_6", "head_on_tile_last_slot", "trip_boundary_1", "trip_boundary_63", "long_between_short",
         "list_fills_a_tile"]


@pytest.mark.parametrize("name", PLAIN)
def test_plain_entries(capi, name):
    _check(capi, name, capi.CARRIED_U64)
    _check(capi, name, capi.CARRIED_U32, mask=0xFFFFFFFF)


def test_hook_refuses_what_the_build_never_passes(capi):
    e0, f0, _ = CASES["len_17"]
    for x in (0, 7):
        with pytest.raises(capi.CarriedError) as err:
            capi.debug_carried_inplace(e0, f0, x)
        assert err.value.status == 1
    with pytest.raises(capi.CarriedError):
        capi.debug_carried_inplace(e0[:0], f0[:0], 3)


# ---- whole builds -------------------------------------------------------------------------------------------------------------
def _zipf(n, seed, nsym=64):
    return W.zipf_corpus(1, n, seed=seed, nsym=nsym)[0][:n]


class _Corpus:
    """one corpus with its oracle (built once) and its patterns"""

    def __init__(self, blob, ds, seed=1):
        from oracle import OracleIndex
        self.blob, self.ds = blob, ds
        self.ids = np.arange(len(ds) - 1, dtype=np.int64) * 3 + 1
        o = OracleIndex()
        o.add_bulk(self.ids, blob, ds)
        o.build(4)
        o.canonicalize()
        self.o_sa = o.sa()
        self.pats = W.sample_patterns(blob, ds, 300, 1, 10, seed=seed, miss_frac=0.1, miss_byte=int(blob[0]) ^ 0x55)
        self.o_rows = o.query_batch(*self.pats, nthreads=4)

    def build(self, capi, **opts):
        g = capi.GpuStringIndex()
        for k, v in dict(VL, profile=1, **opts).items():
            g.set_option(k, v)
        g.add_bulk(self.ids, self.blob, self.ds)
        g.build()
        assert g.stat("self_check_fallbacks") == 0 and g.stat("group_fallbacks") == 0, opts
        assert np.array_equal(g.sa(), self.o_sa), opts
        rows = g.query_batch(*self.pats)
        assert rows[3] == self.o_rows[3] and all(np.array_equal(a, b) for a, b in zip(rows[:3], self.o_rows[:3])), opts
        return g

    def three_ways(self, capi, strictly, **opts):
        """carried_inplace = 1, = 0 and carried_bits = 0: one array (the oracle's), one set of rows, one set of statistics"""
        g1 = self.build(capi, carried_inplace=1, **opts)
        g0 = self.build(capi, carried_inplace=0, **opts)
        gn = self.build(capi, carried_bits=0, **opts)
        ui, uc = g0.stat("unresolved_after_initial"), g0.stat("unresolved_after_carried")
        assert g1.stat("carried_key_bits") == g0.stat("carried_key_bits") > 0 and gn.stat("carried_key_bits") == 0
        assert ui > 0 and g1.stat("unresolved_after_initial") == ui == gn.stat("unresolved_after_initial")
        assert g1.stat("unresolved_after_carried") == uc and gn.stat("unresolved_after_carried") == ui
        assert g1.stat("carried_rounds") == 1 and g0.stat("carried_rounds") == 1 and gn.stat("carried_rounds") == 0
        assert (g1.stat("carried_inplace"), g0.stat("carried_inplace"), gn.stat("carried_inplace")) == (1, 0, 0)
        ua = g1.stat("unresolved_after_inplace")
        assert uc <= ua <= ui and g0.stat("unresolved_after_inplace") == ui
        if strictly:
            assert ua < ui, (ua, ui)
        for name in ("rounds", "ext_rounds", "dbl_rounds", "list_rounds", "group_sorts", "group_sort_fallbacks", "final_depth"):
            assert g1.stat(name) == g0.stat(name), (name, opts)
        p1, p0, pn = g1.profile(), g0.profile(), gn.profile()
        assert "sa_carried_inplace" in p1 and "sa_carried_inplace" not in p0 and "sa_carried_inplace" not in pn
        assert p1["sa_carried_inplace"]["launches"] == 1 and p1["sa_carried_inplace"]["bytes"] >= g1.size
        return g1, g0, gn


@pytest.fixture(scope="module")
def pair_corpus():
    # tests/test_gpu_carried_bits.py's pair corpus: 20 000 pairs of documents that share their first eight symbols, about 41 code
    # bits, and one long document — 33-bit entries, 6 carried bits, ties that part bit by bit
    pairs = np.repeat(_zipf(14 * 20000, 31).reshape(20000, 14), 2, axis=0)
    pairs[1::2, 8:] = _zipf(6 * 20000, 32).reshape(20000, 6)
    blob = np.concatenate([pairs.reshape(-1), _zipf(70000, 33)])
    ds = np.concatenate([np.arange(40001, dtype=np.uint64) * 14, [len(blob)]]).astype(np.uint64)
    return _Corpus(blob, ds)


@pytest.fixture(scope="module")
def ends_corpus():
    # ... and its "document ends inside the carried bits" corpus: documents of 1..12 symbols that are prefixes of longer ones
    rng = np.random.default_rng(5)
    stems = _zipf(14 * 3000, 3).reshape(3000, 14)
    parts, lens = [], []
    for s in stems:
        for k in rng.permutation(np.arange(1, 13)):
            parts.append(s[:k])
            lens.append(k)
    lens.insert(len(lens) // 2, 300000)
    parts.insert(len(parts) // 2, _zipf(300000, 4))
    ds = np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.uint64))]).astype(np.uint64)
    return _Corpus(np.concatenate(parts), ds)


def test_builds_pair_corpus(capi, pair_corpus):
    g1, _, _ = pair_corpus.three_ways(capi, strictly=True)
    assert g1.stat("carried_key_bits") == 6


def test_builds_document_ends_inside_the_carried_bits(capi, ends_corpus):
    g1, _, _ = ends_corpus.three_ways(capi, strictly=False)
    assert g1.stat("carried_key_bits") == 5 and g1.stat("ext_rounds") >= 1


def test_builds_without_group_sort(capi, pair_corpus):
    g1, _, _ = pair_corpus.three_ways(capi, strictly=True, group_sort=0)
    assert g1.stat("group_sorts") == 0


def test_builds_without_list_rounds(capi, pair_corpus):
    g1, _, _ = pair_corpus.three_ways(capi, strictly=True, list_rounds=0)
    assert g1.stat("list_rounds") == 0


def test_builds_three_bucket_groups(capi, pair_corpus):
    g1, _, _ = pair_corpus.three_ways(capi, strictly=True, bucket_group_limit=int(len(pair_corpus.blob) * 0.3))
    assert g1.stat("bucket_groups") >= 3, g1.stat("bucket_groups")


def test_automatic_mode_is_off_below_its_threshold(capi, pair_corpus):
    g = pair_corpus.build(capi)
    assert g.stat("carried_inplace") == 0 and g.stat("carried_rounds") == 1 and "sa_carried_inplace" not in g.profile()
