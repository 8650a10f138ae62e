"""The sort referee (tests/sort_referee.py) pinned on the CPU: against a naive sort of tuples, and every case builder against the
edge it exists for — a case that stops covering its edge fails here, without a GPU."""
import numpy as np
import pytest

from tests import sort_referee as R


def _naive_plain(keys, vals, begin, end):
    m = (1 << (end - begin)) - 1
    order = sorted(range(len(keys)), key=lambda i: ((int(keys[i]) >> begin) & m, i))
    return [int(keys[i]) for i in order], [int(vals[i]) for i in order]


def _naive_split(k32, vals, aux, hi_bits, lead):
    def comp(i):
        return ((int(k32[i]) & ((1 << hi_bits) - 1)) << (8 * lead)) | (int(aux[i]) & ((1 << (8 * lead)) - 1))
    order = sorted(range(len(k32)), key=lambda i: (comp(i), i))
    return [int(k32[i]) for i in order], [int(vals[i]) for i in order], [int(aux[i]) for i in order]


@pytest.mark.parametrize("key_bytes,begin,end", [(8, 0, 64), (8, 0, 1), (8, 7, 8), (8, 5, 41), (8, 40, 64), (4, 0, 32), (4, 3, 29)])
def test_plain_sort_matches_naive(key_bytes, begin, end):
    c = R.bit_range_case(300, key_bytes, begin, end, seed=7)
    vals = np.arange(300, dtype=np.uint32)
    k, v = R.plain_sort(c["keys"], vals, begin, end)
    nk, nv = _naive_plain(c["keys"], vals, begin, end)
    assert [int(x) for x in k] == nk and [int(x) for x in v] == nv
    assert sorted(int(x) for x in k) == sorted(int(x) for x in c["keys"])  # whole keys travel


@pytest.mark.parametrize("aux_bytes,lead,hi_bits", [(1, 0, 9), (1, 1, 32), (2, 1, 8), (2, 2, 24), (4, 0, 1), (4, 3, 31), (4, 4, 32)])
def test_split_sort_matches_naive(aux_bytes, lead, hi_bits):
    c = R.split_case(257, 4, aux_bytes, hi_bits, lead, "uniform", 3840, seed=3)
    c["keys"] &= np.uint32(0xF00000FF)         # few distinct sort keys: ties inside hi_bits, live bits above
    vals = np.arange(257, dtype=np.uint32)
    k, v, a = R.split_sort(c["keys"], vals, c["aux"], hi_bits, lead)
    nk, nv, na = _naive_split(c["keys"], vals, c["aux"], hi_bits, lead)
    assert [int(x) for x in k] == nk and [int(x) for x in v] == nv and [int(x) for x in a] == na


def test_pass_prediction():
    keys = np.array([0x11AA22, 0x33AA44, 0x55AA22], dtype=np.uint64)
    assert R.predict_passes(keys, 0, 24) == (2, 1)
    assert R.predict_passes(keys, 0, 64) == (2, 6)
    assert R.predict_passes(keys, 0, 64, device_hist=True) == (8, 0)
    assert R.predict_passes(keys, 8, 16) == (0, 1)
    assert R.predict_passes(keys[:1], 0, 64) == (0, 8)
    assert R.predict_passes(keys, 0, 24, dbits=5) == (4, 1)   # digits 5 + 5 + 5 + 5 + 4: bits 10..14 = 0b01000 for all three
    assert R.pass_count(0, 64, 4) == R.MAX_PASSES and R.pass_count(0, 64, 3) == 22
    k32 = np.array([1, 2, 3], dtype=np.uint32)
    aux = np.array([0x0105, 0x0205, 0x0305], dtype=np.uint16)
    assert R.predict_passes_split(k32, aux, 9, 2) == (2, 2)
    assert R.predict_passes_split(k32, aux, 9, 1) == (1, 2)
    assert R.predict_passes_split(k32, aux, 9, 1, device_hist=True) == (3, 0)


def test_config_table_and_edge_sizes():
    # by hand from radix_sort(): 1024 x 16, 256 x 18, 256 x 15; key-only 256 x 16 below 2^23 keys, 1024 x 16 from there
    assert R.tile_chunk("pair", 33) == (16384, 1024) and R.tile_chunk("pair", 31) == (16384, 1024)
    assert R.tile_chunk("pair", 36) == (4608, 1152) and R.tile_chunk("pair", 32) == (3840, 960)
    assert R.tile_chunk("pair", 0, n=1000) == (3840, 960) and R.tile_chunk("pair", 0, n=1 << 19) == (4608, 1152)
    assert R.tile_chunk("pair", 0, n=1 << 23) == (16384, 1024)
    assert R.tile_chunk("keyonly", n=(1 << 23) - 1) == (4096, 1024) and R.tile_chunk("keyonly", n=1 << 23) == (16384, 1024)
    # radix_sort_split(): the big tile shrinks to 1024 x 12 for 8-byte values
    assert R.tile_chunk("split", 33, val_bytes=8) == (12288, 768) and R.tile_chunk("split", 33, val_bytes=4) == (16384, 1024)
    assert R.tile_chunk("split", 32, val_bytes=8) == (3840, 960)
    for (kind, v), (nt, ipt) in R.CONFIGS.items():
        assert nt % 64 == 0 and nt * ipt <= 16384
    T, C = 3840, 960
    s = R.edge_sizes(T, C)
    assert s == [1, 2, 63, 64, 65, 959, 960, 961, 2881, 3839, 3840, 3841, 7680, 12481]
    assert [R.tiles(n, T) for n in (T - 1, T, T + 1, 2 * T, 3 * T + C + 1)] == [1, 1, 2, 2, 4]


@pytest.mark.parametrize("key_bytes", [4, 8])
@pytest.mark.parametrize("T", [3840, 4096, 16384])
def test_patterns_reach_their_edges(key_bytes, T):
    bits = 8 * key_bytes
    ones = (1 << bits) - 1
    n = 2 * T + 1029
    k = R.pattern_keys("uniform", n, key_bytes, T)
    assert (k >> (bits - 1)).sum() >= n // 4                       # the top bit is set in at least a quarter of the keys
    assert len(np.unique(k & 0xFF)) == 256 and len(np.unique(k >> (bits - 8))) == 256   # digit 255 occurs in every pass
    assert R.predict_passes(k, 0, bits) == (key_bytes, 0)
    k = R.pattern_keys("ones", n, key_bytes, T)
    assert (k == ones).all()
    k = R.pattern_keys("ones_sparse", n, key_bytes, T)
    other = int((k != ones).sum())
    assert 1 <= other <= n // 25 and R.predict_passes(k, 0, bits)[0] >= 1
    assert int((R.pattern_keys("ones_sparse", 2, key_bytes, T) != ones).sum()) >= 1
    k = R.pattern_keys("one_bit", n, key_bytes, T)
    assert set(np.unique(k)) == {0, 1} and R.predict_passes(k, 0, bits) == (1, key_bytes - 1)
    for name, sign in (("ascending", 1), ("descending", -1)):
        k = R.pattern_keys(name, n, key_bytes, T).astype(np.uint64)
        d = np.diff(k.astype(np.int64) if key_bytes == 4 else (k >> np.uint64(1)).astype(np.int64))
        assert (d * sign > 0).all()
        top = k >> np.uint64(bits - 8)                               # one or two digit runs per tile in the top pass
        assert max(len(np.unique(top[t:t + T])) for t in range(0, n, T)) <= 256 * T // n + 2
        assert (k >> np.uint64(bits - 1)).any()
    for m in (n, T, T + 1, 5, 3 * T):
        k = R.pattern_keys("last_tile_ones", m, key_bytes, T)
        last = (m - 1) // T * T
        assert R.tiles(m, T) == last // T + 1
        assert (k[last:] == ones).all()                              # the last tile's real keys are digit 255 in every pass
        if last:
            assert (k[:last] != ones).any() and R.predict_passes(k, 0, bits) == (key_bytes, 0)


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_every_pattern_exists_at_every_edge_size(key_bytes):
    for T, C in sorted({(nt * ipt, 64 * ipt) for nt, ipt in R.CONFIGS.values()}):
        sizes = R.edge_sizes(T, C)
        assert len(sizes) == 14 and sizes == sorted(sizes) and sizes[0] == 1
        for n in sizes:
            for pattern in R.PATTERNS:
                k = R.pattern_keys(pattern, n, key_bytes, T)
                assert k.dtype.itemsize == key_bytes and len(k) == n
            for val_bytes, aux_bytes in ((4, 1), (4, 2), (4, 4), (8, 1), (8, 2)):
                for pattern in ("uniform", "ones", "one_bit"):
                    c = R.split_case(n, val_bytes, aux_bytes, 9, aux_bytes, pattern, T)
                    assert len(c["keys"]) == n == len(c["aux"]) and c["keys"].dtype == np.uint32 and c["aux"].dtype.itemsize == aux_bytes


@pytest.mark.parametrize("key_bytes,begin,end", [(8, 0, 1), (8, 0, 9), (8, 0, 63), (8, 0, 64), (8, 7, 8), (8, 5, 41), (8, 40, 64),
                                                 (4, 0, 32), (4, 0, 31), (4, 0, 17), (4, 3, 29)])
def test_bit_range_cases_reach_their_edges(key_bytes, begin, end):
    bits = 8 * key_bytes
    n = 3841
    k = R.bit_range_case(n, key_bytes, begin, end)["keys"].astype(np.uint64)
    above = k >> np.uint64(end) if end < 64 else np.zeros(n, dtype=np.uint64)
    below = k & np.uint64((1 << begin) - 1)
    if end < bits:
        assert above.any()
    if begin:
        assert below.any()
    if (begin, end) != (0, bits):
        # keys that tie inside the range differ outside it: a sort that looked at those bits would reorder them
        f = R.sort_field(k, begin, end)
        perm = np.argsort(f, kind="stable")
        fs, ks = f[perm], k[perm]
        tie = fs[1:] == fs[:-1]
        assert tie.sum() >= n // 2 and (ks[1:][tie] != ks[:-1][tie]).any()
        assert not np.array_equal(ks, np.sort(k))


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_skip_cases_reach_their_edges(key_bytes):
    bits = 8 * key_bytes
    n = 7681
    for name in R.SKIP_CASES:
        c = R.skip_case(name, n, key_bytes)
        k = c["keys"]
        cols = R._digits(R.sort_field(k, 0, bits), bits, 8)
        constant = [p for p, col in enumerate(cols) if (col == col[0]).all()]
        if name == "single":
            assert len(k) == 1 and R.predict_passes(k, 0, bits) == (0, key_bytes)
            continue
        assert constant == c["constant_passes"]
        assert R.predict_passes(k, 0, bits) == (key_bytes - len(constant), len(constant))
        assert R.predict_passes(k, 0, bits, device_hist=True) == (key_bytes, 0)
    assert R.skip_case("middle_constant", n, key_bytes)["constant_passes"] == [key_bytes // 2]   # exactly one, in the middle
    assert 0 < key_bytes // 2 < key_bytes - 1


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7])
def test_executed_passes_cases(k):
    c = R.executed_passes_case(7681, k)
    assert R.predict_passes(c["keys"], c["begin"], c["end"]) == (k, 0)
    assert (c["keys"] >> np.uint64(c["end"])).any()


def test_epoch_sequence_wraps_on_first_middle_and_last_pass():
    seq = R.epoch_sequence()
    assert set(seq) == set(R.EPOCH_PASSES)
    wraps, after = R.epoch_wraps(seq)
    assert [w for _, w in wraps] == ["first", "middle", "last"]
    assert sum(seq) > 3 * 255
    drops = [i for i in range(1, len(after)) if after[i] < after[i - 1]]
    assert len(drops) == 3 and drops == [i for i, _ in wraps]
    assert R.epoch_after(0, 255) == (255, None) and R.epoch_after(255, 1) == (1, 0) and R.epoch_after(250, 8) == (3, 5)
    # naive count: executed pass j of a fresh workspace has epoch (j - 1) % 255 + 1
    total = 0
    for k, e in zip(seq, after):
        total += k
        assert e == (total - 1) % 255 + 1


@pytest.mark.parametrize("val_bytes,aux_bytes", [(4, 1), (4, 2), (4, 4), (8, 1), (8, 2)])
def test_split_cases_reach_their_edges(val_bytes, aux_bytes):
    T, _ = R.tile_chunk("split", 33, val_bytes=val_bytes)
    n = T + 1
    for lead in range(aux_bytes + 1):
        for pattern in ("uniform", "ones", "one_bit"):
            c = R.split_case(n, val_bytes, aux_bytes, 9, lead, pattern, T)
            carried = c["aux"].astype(np.uint64) >> np.uint64(8 * lead)
            if lead < aux_bytes:
                assert len(np.unique(carried)) > 16                  # random bits in the carried bytes
            if pattern == "ones":
                assert (c["keys"] == 0xFFFFFFFF).all()
                assert ((c["aux"].astype(np.uint64) & np.uint64((1 << (8 * lead)) - 1)) == (1 << (8 * lead)) - 1).all()
            if pattern == "one_bit" and lead:
                assert set(np.unique(c["aux"].astype(np.uint64) & np.uint64((1 << (8 * lead)) - 1))) == {0, 1}
            assert (c["keys"].astype(np.uint64) >> np.uint64(9)).any() or pattern == "one_bit"   # live key bits above hi_bits
