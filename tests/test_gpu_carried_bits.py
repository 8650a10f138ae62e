"""Carried key bits: where variable-length keys, the records sweep and the segmented last pass run together, the sweep writes
the next X bits of the code stream into the spare bits of every record's auxiliary word, the last pass hands them on in bits
2.. of the flag byte, and the refinement's first round (the carried round) sorts the tied groups on them without reading the
text.  Every build here is checked against the CPU oracle and, array for array and row for row, against the same build with
carried_bits = 0 — which writes exactly the records of a library without the feature."""
import numpy as np
import pytest

from coffeedb_amd import workloads as W

pytestmark = pytest.mark.gpu

VL = dict(force_big_path=1, vl_keys=40)


@pytest.fixture(scope="module")
def G():
    from coffeedb_amd import capi
    capi.load_library()
    return capi.GpuStringIndex


def _docs(nsmall, small_len, big_len):
    """many small documents and one long one: the entry width is bit_width(documents) + bit_width(longest) (cdb_layout_rule)"""
    lens = np.full(nsmall, small_len, dtype=np.uint64)
    lens[nsmall // 3] = big_len
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _zipf(n, seed, nsym=64):
    return W.zipf_corpus(1, n, seed=seed, nsym=nsym)[0][:n]


def _expected_x(nd, longest, cap=-1):
    from coffeedb_amd import capi
    bits, _, width, off = capi.layout_rule(nd, longest)
    x = max(0, min(40 - (bits + off), 6, 64 - 7 - 39))
    return (x if cap < 0 else min(x, cap)), bits + off, width


class _Case:
    """one corpus with its oracle (built once) and its patterns; build() checks one option set against both"""

    def __init__(self, blob, ds, npat=300, seed=1):
        from oracle import OracleIndex
        self.blob, self.ds = blob, ds
        self.ids = np.arange(len(ds) - 1, dtype=np.int64) * 3 + 1
        o = OracleIndex()
        o.add_bulk(self.ids, blob, ds)
        o.build(4)
        o.canonicalize()
        self.o_sa = o.sa()
        self.shape = (o.size, o.bits, o.mask, o.sa_width)
        self.pats = W.sample_patterns(blob, ds, npat, 1, 10, seed=seed, miss_frac=0.1, miss_byte=int(blob[0]) ^ 0x55)
        self.o_rows = o.query_batch(*self.pats, nthreads=4)
        self.lens = np.diff(ds)

    def build(self, G, **opts):
        g = G()
        for k, v in opts.items():
            g.set_option(k, v)
        g.add_bulk(self.ids, self.blob, self.ds)
        g.build()
        assert g.stat("self_check_fallbacks") == 0 and g.stat("group_fallbacks") == 0, opts
        assert (g.size, g.bits, g.mask, g.sa_width) == self.shape
        sa = g.sa()
        assert np.array_equal(sa, self.o_sa), opts
        rows = g.query_batch(*self.pats)
        assert rows[3] == self.o_rows[3] and all(np.array_equal(a, b) for a, b in zip(rows[:3], self.o_rows[:3])), opts
        return g, sa, rows

    def pair(self, G, x, split=True, **opts):
        """the build with carried bits (x of them expected) and the same build without: same array, same rows"""
        for k, v in VL.items():  # (the sweep with variable-length keys, unless the caller says otherwise)
            opts.setdefault(k, v)
        g, sa, rows = self.build(G, **opts)
        g0, sa0, rows0 = self.build(G, **dict(opts, carried_bits=0))
        assert np.array_equal(sa, sa0) and rows[3] == rows0[3] and all(np.array_equal(a, b) for a, b in zip(rows[:3], rows0[:3])), opts
        assert g.stat("vl_key_bits") == 40 and g.stat("sweep_records") == 1 and g.stat("segmented") == 1, opts
        assert g0.stat("vl_key_bits") == 40 and g0.stat("carried_key_bits") == 0 and g0.stat("carried_rounds") == 0
        assert g.stat("carried_key_bits") == x, (x, g.stat("carried_key_bits"), opts)
        ui, uc = g.stat("unresolved_after_initial"), g.stat("unresolved_after_carried")
        assert ui == g0.stat("unresolved_after_initial") == g0.stat("unresolved_after_carried")
        if x > 0 and ui > 0:
            assert g.stat("carried_rounds") == 1
            assert uc < ui if split else uc <= ui, (ui, uc, opts)
        else:
            assert g.stat("carried_rounds") == 0 and uc == ui
        # the round statistics count text and doubling rounds only
        assert g.stat("list_rounds") == (max(0, g.stat("ext_rounds") - 1) if opts.get("list_rounds", 1) else 0), opts
        assert g.stat("group_sort_fallbacks") == g0.stat("group_sort_fallbacks"), opts
        return g, g0


@pytest.mark.parametrize("nd,longest,width", [(40000, 70000, 33), (40000, 300000, 35), (70000, 1100000, 38), (70000, 2100000, 39),
                                              (140000, 2100000, 40)])
def test_entry_widths(G, nd, longest, width):
    # 33 / 35 / 38 / 39 / 40 entry bits leave room for 6 (capped) / 5 / 2 / 1 / 0 carried bits above the entry's high bits
    x, w, sa_width = _expected_x(nd, longest)
    assert w == width and sa_width == 8 and x == {33: 6, 35: 5, 38: 2, 39: 1, 40: 0}[width]
    ds = _docs(nd, 3, longest)
    c = _Case(_zipf(int(ds[-1]), 11 + width), ds)
    g, g0 = c.pair(G, x)
    if width == 40:
        assert g.stat("carried_rounds") == 0 and g.stat("rounds") == g0.stat("rounds")


def test_document_ends_inside_the_carried_bits(G):
    # documents of 1..12 symbols that are prefixes of longer ones: their code streams end inside the key or inside the carried
    # bits, where the sweep pads with zeros — the shorter document comes first, and the tie between an ended suffix and one
    # that goes on with zero bits stays open for the text round
    rng = np.random.default_rng(5)
    stems = _zipf(14 * 3000, 3).reshape(3000, 14)
    parts, lens = [], []
    for s in stems:
        for k in rng.permutation(np.arange(1, 13)):
            parts.append(s[:k])
            lens.append(k)
    lens.insert(len(lens) // 2, 300000)                     # (the long document: 35-bit entries)
    parts.insert(len(parts) // 2, _zipf(300000, 4))
    ds = np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.uint64))]).astype(np.uint64)
    x, w, _ = _expected_x(len(lens), 300000)
    assert x == 5 and w == 35
    c = _Case(np.concatenate(parts), ds)
    g, _ = c.pair(G, x)
    assert g.stat("ext_rounds") >= 1                        # groups of equal short documents are closed by a text round


@pytest.mark.parametrize("copies", [2, 3000])
def test_duplicated_documents(G, copies):
    # groups that never resolve: with thousands of copies the group sort gives up — in the carried round now, once, as the first
    # text round does without carried bits
    doc = _zipf(60, 21)
    n_other = 300000
    # (beside them pairs of documents that share eight symbols, about 41 code bits: some part inside the carried bits)
    npair = (33000 - copies - 1) // 2                      # (33 000 documents: 16 document bits + 19 offset bits)
    pairs = np.repeat(_zipf(14 * npair, 23).reshape(npair, 14), 2, axis=0)
    pairs[1::2, 8:] = _zipf(6 * npair, 24).reshape(npair, 6)
    parts = [doc] * copies + [_zipf(n_other, 22), pairs.reshape(-1)]
    lens = [60] * copies + [n_other] + [14] * (2 * npair)
    ds = np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.uint64))]).astype(np.uint64)
    x, w, _ = _expected_x(len(lens), n_other)
    assert x == 5
    c = _Case(np.concatenate(parts), ds)
    g, g0 = c.pair(G, x)
    if copies > 100:
        assert g.stat("group_sort_fallbacks") == 1 and g0.stat("group_sort_fallbacks") == 1


def test_one_symbol_text(G):
    # the deep-LCP case: one symbol throughout (and one other byte at the very end, so that a code exists at all) — every
    # carried value is equal and the carried round splits next to nothing; doubling takes over behind it
    # (half a million one-symbol documents and one of 8192: 20 + 14 entry bits, and an oracle whose compares stay short)
    ds = _docs(524288, 1, 8192)
    blob = np.full(int(ds[-1]), 0x61, dtype=np.uint8)
    blob[-1] = 0x62
    c = _Case(blob, ds, npat=100)
    x, w, _ = _expected_x(524288, 8192)
    assert x == 6 and w == 34
    g, g0 = c.pair(G, x, split=False)
    assert g.stat("rounds") >= 2


def test_skewed_code_lengths(G):
    # one symbol in two, the rest falling off geometrically: code words from 1-2 bits to the 7-bit limit, so that 39 + X bits
    # span from 6 to more than 20 symbols
    rng = np.random.default_rng(9)
    p = np.concatenate([[0.5, 0.2], 0.3 * 0.8 ** np.arange(60) / np.sum(0.8 ** np.arange(60))])
    ds = _docs(40000, 3, 300000)
    blob = (0x30 + rng.choice(len(p), size=int(ds[-1]), p=p)).astype(np.uint8)
    c = _Case(blob, ds)
    x, _, _ = _expected_x(40000, 300000)
    g, _ = c.pair(G, x)
    assert g.stat("vl_avg_len") < 4.0                      # (Zipf-64: 5.19)


def test_options_give_the_same_array(G):
    # carried_bits = 1..6 as a cap, list_rounds = 0, group_sort = 0 and two or three bucket groups on one shape
    # (20 000 pairs of documents that share their first eight symbols, about 41 code bits, and one long document:
    #  33-bit entries, up to 6 carried bits, and ties that part bit by bit)
    pairs = np.repeat(_zipf(14 * 20000, 31).reshape(20000, 14), 2, axis=0)
    pairs[1::2, 8:] = _zipf(6 * 20000, 32).reshape(20000, 6)
    blob = np.concatenate([pairs.reshape(-1), _zipf(70000, 33)])
    ds = np.concatenate([np.arange(40001, dtype=np.uint64) * 14, [len(blob)]]).astype(np.uint64)
    n = len(blob)
    c = _Case(blob, ds)
    open_after = []
    for cap in range(1, 7):
        x, _, _ = _expected_x(40001, 70000, cap)
        assert x == cap
        g, _ = c.pair(G, x, carried_bits=cap, **VL)
        open_after.append(g.stat("unresolved_after_carried"))
    assert all(a >= b for a, b in zip(open_after, open_after[1:])) and open_after[0] > open_after[-1], open_after
    c.pair(G, 6, list_rounds=0, **VL)
    g, _ = c.pair(G, 6, group_sort=0, **VL)
    assert g.stat("group_sorts") == 0
    g, _ = c.pair(G, 6, force_doubling=1, **VL)
    assert g.stat("isa_built") == 1
    for frac in (0.55, 0.4):
        g, _ = c.pair(G, 6, bucket_group_limit=int(n * frac), **VL)
        assert g.stat("bucket_groups") >= 2, g.stat("bucket_groups")
    # without the sweep there are no variable-length keys: the build takes dense keys and carries nothing
    g, _, _ = c.build(G, sweep_records=0, **VL)
    assert g.stat("vl_key_bits") == 0 and g.stat("carried_key_bits") == 0 and g.stat("carried_rounds") == 0


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_mid_size_with_drawn_carried_bits(G, seed):
    # the mid-size family of tests/test_gpu_fuzz.py (documents of hundreds of bytes, tiles that take the fast phase B of the
    # sweep, several bucket groups) on skewed text, with carried_bits drawn beside the options that meet it
    rng = np.random.default_rng(77000 + seed)
    nd = int(rng.integers(3000, 12000))
    mean = int(rng.integers(40, 300))
    lens = rng.integers(mean // 2, mean * 3 // 2 + 2, size=nd).astype(np.uint64)
    if rng.random() < 0.3: lens[rng.integers(0, nd, size=nd // 50)] = 0
    if rng.random() < 0.85: lens[int(rng.integers(0, nd))] = int(rng.integers(1 << 17, 1 << 20))
    while int(lens.sum()) > 2_500_000: lens = lens[: len(lens) * 3 // 4]
    ds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(ds[-1])
    blob = _zipf(n, int(rng.integers(1 << 30)), nsym=int(rng.integers(8, 90)))
    if rng.random() < 0.3:                                   # long repeats: groups the key and the carried bits cannot resolve
        q = n // 4
        blob[2 * q:3 * q] = blob[:q]
    opts = {"carried_bits": int(rng.integers(-1, 7))}
    if rng.random() < 0.7: opts["bucket_group_limit"] = max(1, int(n * rng.uniform(0.08, 1.0)))
    if rng.random() < 0.2: opts["vl_keys"] = int(rng.choice([1, 32, 48, 56]))
    if rng.random() < 0.2: opts["pack_sa"] = 0
    if rng.random() < 0.15: opts["plain_tile_order"] = 1
    if rng.random() < 0.15: opts["force_doubling"] = 1
    if rng.random() < 0.2: opts["group_sort"] = 0
    if rng.random() < 0.2: opts["list_rounds"] = 0
    for k, v in VL.items():
        opts.setdefault(k, v)
    c = _Case(blob, ds, npat=100, seed=seed)
    g, sa, _ = c.build(G, **opts)
    opts0 = dict(opts, carried_bits=0)
    g0, sa0, _ = c.build(G, **opts0)
    info = (seed, len(lens), n, opts, g.sa_width, g.stat("vl_key_bits"), g.stat("carried_key_bits"), g.stat("bucket_groups"))
    assert np.array_equal(sa, sa0), info
    assert g.stat("bucketed") == 1 and g0.stat("carried_key_bits") == 0, info
    assert 0 <= g.stat("carried_key_bits") <= (6 if opts["carried_bits"] < 0 else opts["carried_bits"]), info
    assert g.stat("unresolved_after_carried") <= g.stat("unresolved_after_initial") == g0.stat("unresolved_after_initial"), info
    assert g.proof_wait(60_000) == 2 and g.stat("self_check_fallbacks") == 0, info
    g.close()
    g0.close()
