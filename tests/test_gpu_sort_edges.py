"""The radix-sort primitive (radix_sort.h) at its tile, digit and workspace edges, called as the library calls it
(cdb_debug_radix_sort_ex / cdb_debug_radix_sort_split) and compared with the numpy referee of tests/sort_referee.py.

Every comparison is integer equality of keys and of values; values are arange(n), so equal values mean a stable sort."""
import numpy as np
import pytest

from tests import sort_referee as R

pytestmark = pytest.mark.gpu

E_INVALID, E_INTERNAL = 1, 3
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(_SIGNED[a.dtype])).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _vals(n, val_bytes):
    return np.arange(n, dtype=R._udtype(val_bytes)) if val_bytes else None


def run_plain(keys, val_bytes, begin, end, dbits=8, variant=0, flags=0, ws=None):
    """(keys, values, result record) after the hook; the library sorts on its own stream: synchronise before and after"""
    import torch
    from coffeedb_amd import capi
    vals = _vals(len(keys), val_bytes)
    k = _dev(keys)
    v = _dev(vals) if val_bytes else None
    torch.cuda.synchronize()
    try:
        r = capi.debug_radix_sort_ex(k.data_ptr(), v.data_ptr() if val_bytes else 0, len(keys), keys.dtype.itemsize, val_bytes, begin,
                                     end, dbits, variant, flags, ws)
    finally:
        torch.cuda.synchronize()
        run_plain.last = (_host(k, keys.dtype), _host(v, vals.dtype) if val_bytes else None)
    return run_plain.last[0], run_plain.last[1], r


def _pattern_flags(pattern, val_bytes):
    """all-ones keys have every digit constant: with the histograms left on the device the passes run all the same, and real
    digit 255 meets the padding in each of them.  (Pair sorts only: radix_sort() hands device histograms to no key-only
    configuration, and the hook refuses the flag there.)"""
    from coffeedb_amd import capi
    return capi.SORT_DEVICE_HIST if pattern == "ones" and val_bytes else 0


def check_plain(keys, val_bytes, begin, end, what, **kw):
    vals = _vals(len(keys), val_bytes)
    ek, ev = R.plain_sort(keys, vals, begin, end)
    gk, gv, r = run_plain(keys, val_bytes, begin, end, **kw)
    assert np.array_equal(gk, ek), ("keys", what, len(keys), kw)
    if val_bytes:
        assert np.array_equal(gv, ev), ("values", what, len(keys), kw)
    return r


def run_split(c, val_bytes, variant=0, flags=0, ws=None):
    import torch
    from coffeedb_amd import capi
    n = len(c["keys"])
    k, v, a = _dev(c["keys"]), _dev(_vals(n, val_bytes)), _dev(c["aux"])
    torch.cuda.synchronize()
    r = capi.debug_radix_sort_split(k.data_ptr(), v.data_ptr(), a.data_ptr(), n, val_bytes, c["aux"].dtype.itemsize, c["hi_bits"],
                                    c["lead"], variant, flags, ws)
    torch.cuda.synchronize()
    return _host(k, np.uint32), _host(v, R._udtype(val_bytes)), _host(a, c["aux"].dtype), r


def check_split(c, val_bytes, **kw):
    n = len(c["keys"])
    ek, ev, ea = R.split_sort(c["keys"], _vals(n, val_bytes), c["aux"], c["hi_bits"], c["lead"])
    gk, gv, ga, r = run_split(c, val_bytes, **kw)
    assert np.array_equal(gk, ek), ("keys", c["edge"], n, kw)
    assert np.array_equal(gv, ev), ("values", c["edge"], n, kw)
    assert np.array_equal(ga, ea), ("auxiliary words", c["edge"], n, kw)
    return r


# ------------------------------------------------------------------------------------------------------------------------
# tile edges
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(R.PRODUCTION_VARIANTS) + [31, 0] + list(R.AB_VARIANTS))
@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("key_bytes", [8, 4])
def test_pair_sort_tile_edges(key_bytes, val_bytes, variant):
    if key_bytes == 4 and variant in R.AB_VARIANTS:
        from coffeedb_amd import capi
        with pytest.raises(capi.SortError) as e:       # 4 and 41 stay 64-bit only
            run_plain(np.zeros(4, dtype=np.uint32), val_bytes, 0, 32, variant=variant)
        assert e.value.status == E_INVALID
        return
    T, C = R.tile_chunk("pair", variant, n=1)          # (31 without the grouped flag runs as 33: the same tile)
    for n in R.edge_sizes(T, C):
        for pattern in R.PATTERNS:
            r = check_plain(R.pattern_keys(pattern, n, key_bytes, T), val_bytes, 0, 8 * key_bytes, pattern, variant=variant,
                            flags=_pattern_flags(pattern, val_bytes))
            if pattern == "ones":
                assert r["passes_run"] == key_bytes


@pytest.mark.parametrize("variant", [0, 21])
@pytest.mark.parametrize("key_bytes", [8, 4])
def test_key_only_tile_edges(key_bytes, variant):
    T, C = R.tile_chunk("keyonly", n=1)
    assert T == 4096
    for n in R.edge_sizes(T, C):
        for pattern in R.PATTERNS:
            r = check_plain(R.pattern_keys(pattern, n, key_bytes, T), 0, 0, 8 * key_bytes, pattern, variant=variant)
            if pattern == "ones":
                assert r["passes_run"] == 0                  # (digit 255 beside the padding: "ones_sparse", "last_tile_ones")


# ------------------------------------------------------------------------------------------------------------------------
# bit ranges and digit widths
# ------------------------------------------------------------------------------------------------------------------------
RANGES = {8: [(0, 1), (0, 9), (0, 63), (0, 64), (7, 8), (5, 41), (40, 64)], 4: [(0, 32), (0, 31), (0, 17), (3, 29)]}


@pytest.mark.parametrize("variant", [32, 33])
@pytest.mark.parametrize("key_bytes", [8, 4])
def test_bit_ranges_and_digit_widths(key_bytes, variant):
    T, C = R.tile_chunk("pair", variant)
    for n in (T + 1, 3 * T + C + 1):
        for begin, end in RANGES[key_bytes]:
            c = R.bit_range_case(n, key_bytes, begin, end)
            for dbits in (8, 7, 5, 4, 2):
                if R.pass_count(begin, end, dbits) > R.MAX_PASSES:
                    continue
                r = check_plain(c["keys"], 4, begin, end, c["edge"], dbits=dbits, variant=variant)
                assert (r["passes_run"], r["passes_skipped"]) == R.predict_passes(c["keys"], begin, end, dbits), (c["edge"], dbits)


@pytest.mark.parametrize("variant", [32, 33])
def test_pass_limit(variant):
    from coffeedb_amd import capi
    T, C = R.tile_chunk("pair", variant)
    for n in (T + 1, 3 * T + C + 1):
        keys = R.pattern_keys("uniform", n, 8, T)
        assert R.pass_count(0, 64, 4) == R.MAX_PASSES
        r = check_plain(keys, 8, 0, 64, "16 passes", dbits=4, variant=variant)
        assert r["passes_run"] == 16
        for flags in (0, capi.SORT_DEVICE_HIST):
            with pytest.raises(capi.SortError) as e:       # 22 passes: refused before anything is touched
                run_plain(keys, 8, 0, 64, dbits=3, variant=variant, flags=flags)
            assert e.value.status == E_INVALID             # (the status Error carries: the caller's mistake)
            gk, gv = run_plain.last
            assert np.array_equal(gk, keys) and np.array_equal(gv, _vals(n, 8))


# ------------------------------------------------------------------------------------------------------------------------
# skipped passes
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SKIP_CASES)
@pytest.mark.parametrize("key_bytes", [8, 4])
def test_skipped_passes(key_bytes, name):
    from coffeedb_amd import capi
    T, C = R.tile_chunk("pair", 32)
    c = R.skip_case(name, 2 * T + C + 1, key_bytes)
    keys, bits = c["keys"], 8 * key_bytes
    for val_bytes in (4, 0):
        r = check_plain(keys, val_bytes, 0, bits, name, variant=32)
        assert (r["passes_run"], r["passes_skipped"]) == R.predict_passes(keys, 0, bits), name
        if name in ("all_equal", "single"):
            assert r["passes_run"] == 0 and r["key_result"] == 0 and r["value_result"] == 0   # both arrays untouched
        if not val_bytes:
            with pytest.raises(capi.SortError) as e:       # (no key-only configuration takes device histograms)
                run_plain(keys, 0, 0, bits, variant=32, flags=capi.SORT_DEVICE_HIST)
            assert e.value.status == E_INVALID
            continue
        # the same input with the histograms left on the device: nothing skipped (a pass in which every key of every tile has
        # one digit), same result
        r = check_plain(keys, val_bytes, 0, bits, name, variant=32, flags=capi.SORT_DEVICE_HIST)
        assert (r["passes_run"], r["passes_skipped"]) == (key_bytes, 0) == R.predict_passes(keys, 0, bits, device_hist=True)


# ------------------------------------------------------------------------------------------------------------------------
# spare value buffer
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val_bytes", [4, 8])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7])
def test_spare_value_buffer(k, val_bytes):
    from coffeedb_amd import capi
    T, C = R.tile_chunk("pair", 32)
    c = R.executed_passes_case(2 * T + C + 1, k)
    for flags in (0, capi.SORT_SPARE_VALUES, capi.SORT_SPARE_VALUES | capi.SORT_DEVICE_HIST):
        r = check_plain(c["keys"], val_bytes, c["begin"], c["end"], c["edge"], variant=32, flags=flags)
        assert r["passes_run"] == k and r["key_result"] == (k & 1)
        if (flags & capi.SORT_SPARE_VALUES) and (k & 1) and k >= 3:
            assert r["value_result"] == 0 and r["key_result"] == 1     # v0 -> spare -> v1 -> ... -> v0
        else:
            assert r["value_result"] == r["key_result"]


# ------------------------------------------------------------------------------------------------------------------------
# big key-only tiles
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bytes,n,grouped", [(8, 1 << 23, False), (4, 1 << 23, False), (8, (1 << 23) + 16384 + 5, False),
                                                 (4, (1 << 23) + 16384 + 5, False), (8, (1 << 23) + 16384 + 5, True)])
def test_big_key_only_tiles(key_bytes, n, grouped):
    from coffeedb_amd import capi
    T, _ = R.tile_chunk("keyonly", n=n)
    assert T == 16384 and R.tiles(n, T) == (512 if n == 1 << 23 else 514)
    keys = R.pattern_keys("uniform", n, key_bytes, T)
    gk, _, r = run_plain(keys, 0, 0, 8 * key_bytes, flags=capi.SORT_GROUPED if grouped else 0)
    assert np.array_equal(gk, np.sort(keys, kind="stable"))
    assert r["passes_run"] == key_bytes
    if grouped:
        print(f"big key-only grouped: fell_back={r['fell_back']}")


# ------------------------------------------------------------------------------------------------------------------------
# grouped (XCD-aware) tile order
# ------------------------------------------------------------------------------------------------------------------------
GROUPED_TILES = [1, 7, 8, 9, 63, 64, 65, 129]


@pytest.mark.parametrize("whole", GROUPED_TILES)
def test_grouped_tile_order_pairs(whole):
    from coffeedb_amd import capi
    T, _ = R.tile_chunk("pair", 31)
    fell = 0
    for n in (whole * T, whole * T + 5):
        assert R.tiles(n, T) == whole + (n > whole * T)
        for pattern in ("uniform", "ones"):
            keys = R.pattern_keys(pattern, n, 8, T)
            r = check_plain(keys, 4, 0, 64, pattern, variant=31, flags=capi.SORT_GROUPED | _pattern_flags(pattern, 4))
            assert r["passes_run"] == 8
            fell += r["fell_back"]
    # the same input in plain ticket order: the two tile orders agree (both equal the referee's result)
    r = check_plain(R.pattern_keys("uniform", whole * T + 5, 8, T), 4, 0, 64, "plain order", variant=31)
    assert r["fell_back"] == 0
    print(f"grouped pairs, {whole} tiles: {fell} of 4 sorts fell back to plain ticket order")


@pytest.mark.parametrize("whole", GROUPED_TILES)
def test_grouped_tile_order_split(whole):
    from coffeedb_amd import capi
    T, _ = R.tile_chunk("split", 31, val_bytes=4)
    fell = 0
    for n in (whole * T, whole * T + 5):
        for pattern in ("uniform", "ones"):
            c = R.split_case(n, 4, 2, 24, 2, pattern, T)
            fell += check_split(c, 4, variant=31, flags=capi.SORT_GROUPED | capi.SORT_DEVICE_HIST)["fell_back"]
    r = check_split(R.split_case(whole * T + 5, 4, 2, 24, 2, "uniform", T), 4, variant=31, flags=capi.SORT_DEVICE_HIST)
    assert r["fell_back"] == 0
    print(f"grouped split records, {whole} tiles: {fell} of 4 sorts fell back to plain ticket order")


# ------------------------------------------------------------------------------------------------------------------------
# workspace lifetime
# ------------------------------------------------------------------------------------------------------------------------
def test_workspace_epoch_wraps():
    from coffeedb_amd import capi
    T, _ = R.tile_chunk("pair", 32)
    n = 2 * T + 1
    seq = R.epoch_sequence()
    wraps, after = R.epoch_wraps(seq)
    assert [w for _, w in wraps] == ["first", "middle", "last"]
    end_of = {8: 64, 7: 56, 5: 40}
    rng = np.random.default_rng(5)
    drops, prev = 0, 0
    with capi.DebugSortWorkspace() as ws:
        for i, k in enumerate(seq):
            keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
            r = check_plain(keys, 4, 0, end_of[k], f"sort {i} of the epoch sequence", variant=32, ws=ws)
            assert r["passes_run"] == k and r["epoch"] == after[i], (i, k)
            drops += r["epoch"] < prev
            prev = r["epoch"]
    assert drops == 3


def test_workspace_status_growth_and_tile_sizes():
    from coffeedb_amd import capi
    variants = [32, 36, 33]
    rng = np.random.default_rng(6)
    epochs = []
    capi.load_library().cdb_release_cached_memory()   # (no cached block larger than asked for: the status array has its exact size)
    with capi.DebugSortWorkspace() as ws:
        for i, ntiles in enumerate([200, 0, 3, 400, 2]):
            v = variants[i % 3]
            T, _ = R.tile_chunk("pair", v)
            n = ntiles * T if ntiles else 1
            keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
            r = check_plain(keys, 8, 0, 64, f"{ntiles} tiles of variant {v}", variant=v, ws=ws)
            assert r["passes_run"] == (8 if ntiles else 0)
            epochs.append(r["epoch"])
    # 8 passes each; the one-key sort runs none; the 400-tile sort grows the status array, which resets the epoch
    assert epochs == [8, 8, 16, 8, 16]


def test_workspace_across_key_types_and_split_records():
    from coffeedb_amd import capi
    T, C = R.tile_chunk("pair", 32)
    n = 3 * T + C + 1
    with capi.DebugSortWorkspace() as ws:
        for rep in range(2):
            check_plain(R.pattern_keys("uniform", n, 4, T, seed=rep), 0, 0, 32, "key-only 32-bit", ws=ws)
            check_plain(R.pattern_keys("uniform", n, 8, T, seed=rep), 8, 0, 64, "64-bit pairs", variant=32, ws=ws)
            check_split(R.split_case(n, 4, 2, 24, 2, "uniform", T, seed=rep), 4, variant=32, ws=ws)
            check_split(R.split_case(n, 8, 1, 32, 1, "uniform", T, seed=rep), 8, variant=33, flags=capi.SORT_DEVICE_HIST, ws=ws)


@pytest.mark.parametrize("variant", [32, 33])
def test_poisoned_sort_leaves_buffers_alone(variant):
    from coffeedb_amd import capi
    T, C = R.tile_chunk("pair", variant)
    n = 3 * T + C + 1
    keys = R.pattern_keys("uniform", n, 8, T)
    with capi.DebugSortWorkspace() as ws:
        check_plain(keys, 4, 0, 64, "before", variant=variant, ws=ws)
        with pytest.raises(capi.SortError) as e:
            run_plain(keys, 4, 0, 64, variant=variant, flags=capi.SORT_POISON, ws=ws)
        assert e.value.status == E_INTERNAL
        gk, gv = run_plain.last
        assert np.array_equal(gk, keys) and np.array_equal(gv, _vals(n, 4))   # buffers 0 bit-identical to the input
        check_plain(keys, 4, 0, 64, "after", variant=variant, ws=ws)
        # under the grouped flag the hook does what the build does: restore, plain order, report
        r = check_plain(keys, 4, 0, 64, "poisoned, grouped", variant=31, flags=capi.SORT_POISON | capi.SORT_GROUPED, ws=ws)
        assert r["fell_back"] == 1


# ------------------------------------------------------------------------------------------------------------------------
# split records
# ------------------------------------------------------------------------------------------------------------------------
HI_BITS = [1, 8, 9, 24, 31, 32]


@pytest.mark.parametrize("variant", [32, 33])
@pytest.mark.parametrize("val_bytes,aux_bytes", [(4, 1), (4, 2), (4, 4), (8, 1), (8, 2)])
def test_split_records(val_bytes, aux_bytes, variant):
    from coffeedb_amd import capi
    T, C = R.tile_chunk("split", variant, val_bytes=val_bytes)
    assert T == (3840 if variant == 32 else (12288 if val_bytes == 8 else 16384))
    i = 0
    for n in R.edge_sizes(T, C):
        for lead in range(aux_bytes + 1):
            # every size meets every lead; hi_bits, pattern and the histograms' side rotate through the sizes
            hi_bits = HI_BITS[i % len(HI_BITS)]
            pattern = ("uniform", "ones", "one_bit")[i % 3]
            device = (i // 3) & 1
            i += 1
            c = R.split_case(n, val_bytes, aux_bytes, hi_bits, lead, pattern, T)
            r = check_split(c, val_bytes, variant=variant, flags=capi.SORT_DEVICE_HIST if device else 0)
            assert (r["passes_run"], r["passes_skipped"]) == R.predict_passes_split(c["keys"], c["aux"], hi_bits, lead, bool(device)), c["edge"]


@pytest.mark.parametrize("val_bytes,aux_bytes", [(4, 1), (4, 2), (4, 4), (8, 1), (8, 2)])
def test_split_records_hi_bits_and_histograms(val_bytes, aux_bytes):
    from coffeedb_amd import capi
    T, C = R.tile_chunk("split", 32, val_bytes=val_bytes)
    n = 3 * T + C + 1
    for hi_bits in HI_BITS:
        for lead in (0, aux_bytes):
            for pattern in ("uniform", "ones", "one_bit"):
                c = R.split_case(n, val_bytes, aux_bytes, hi_bits, lead, pattern, T)
                for flags in (0, capi.SORT_DEVICE_HIST):
                    check_split(c, val_bytes, variant=32, flags=flags)
