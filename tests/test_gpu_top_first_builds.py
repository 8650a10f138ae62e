"""The top-digit-first form of the segmented sort (radix_sort.h: radix_sort_top_first; option top_digit_first) in whole builds:
the same corpus built with the form on and off must give one suffix array (the CPU oracle's), one set of query rows and one set
of refinement statistics, the statistics and the profile must say which form ran, and a build the form does not apply to (dense
keys, bytes >= 0x80 in the reference's order, 8-bit aux words) must report top_first = 0 and build as before."""
import numpy as np
import pytest

from coffeedb_amd import workloads as W

pytestmark = pytest.mark.gpu

VL = dict(force_big_path=1, vl_keys=40)
SAME = ("unresolved_after_initial", "unresolved_after_inplace", "unresolved_after_carried", "carried_rounds", "carried_key_bits", "rounds",
        "ext_rounds", "dbl_rounds", "final_depth", "bucket_groups", "vl_key_bits")
TOP_KERNELS = ("rs_seg_hist_top", "rs_seg_top_w16_t16384", "rs_seg_hist_cells")


@pytest.fixture(scope="module")
def capi():
    from coffeedb_amd import capi
    capi.load_library()
    return capi


def _zipf(n, seed, nsym=64):
    return W.zipf_corpus(1, n, seed=seed, nsym=nsym)[0][:n]


class _Corpus:
    def __init__(self, blob, ds, seed=1):
        from oracle import OracleIndex
        self.blob, self.ds = blob, ds
        self.ids = np.arange(len(ds) - 1, dtype=np.int64) * 3 + 1
        o = OracleIndex()
        o.add_bulk(self.ids, blob, ds)
        o.build(4)
        o.canonicalize()
        self.o_sa = o.sa()
        self.pats = W.sample_patterns(blob, ds, 200, 1, 10, seed=seed, miss_frac=0.1, miss_byte=int(blob[0]) ^ 0x55)
        self.o_rows = o.query_batch(*self.pats, nthreads=4)

    def build(self, capi, **opts):
        g = capi.GpuStringIndex()
        for k, v in dict(profile=1, **opts).items():
            g.set_option(k, v)
        g.add_bulk(self.ids, self.blob, self.ds)
        g.build()
        assert g.stat("group_fallbacks") == 0, opts
        assert np.array_equal(g.sa(), self.o_sa), opts
        rows = g.query_batch(*self.pats)
        assert rows[3] == self.o_rows[3] and all(np.array_equal(a, b) for a, b in zip(rows[:3], self.o_rows[:3])), opts
        assert g.proof_wait(60_000) == 2 and g.stat("self_check_fallbacks") == 0, opts
        return g

    def on_and_off(self, capi, **opts):
        g1 = self.build(capi, top_digit_first=1, **opts)
        g0 = self.build(capi, top_digit_first=0, **opts)
        assert (g1.stat("top_first"), g0.stat("top_first")) == (1, 0), opts
        assert 0 < g1.stat("top_first_cells") <= 256 * 256 and g0.stat("top_first_cells") == 0
        for name in SAME:
            assert g1.stat(name) == g0.stat(name), (name, g1.stat(name), g0.stat(name), opts)
        p1, p0 = g1.profile(), g0.profile()
        groups = g1.stat("bucket_groups")
        for k in TOP_KERNELS:
            assert k in p1 and k not in p0 and p1[k]["launches"] == groups, (k, opts)
        assert "rs_seg_hist" in p0 and "rs_seg_hist" not in p1
        assert p1["rs_seg_k32_v32_w8_t16384"]["launches"] == 3 * groups and "rs_seg_k32_v32_w16_t16384" not in p1
        assert p0["rs_seg_k32_v32_w16_t16384"]["launches"] == 4 * groups
        assert p1["rs_seg_final_w8_t16384"]["launches"] == groups and p0["rs_seg_final_w16_t16384"]["launches"] == groups
        return g1, g0


@pytest.fixture(scope="module")
def pair_corpus():
    # tests/test_gpu_carried_bits.py's pair corpus at 2^20 bytes: 20 000 pairs of documents that share their first eight symbols (ties
    # the 40-bit key leaves open: groups of equal keys in most cells) and one long document; 35-bit entries, 5 carried bits
    pairs = np.repeat(_zipf(14 * 20000, 31).reshape(20000, 14), 2, axis=0)
    pairs[1::2, 8:] = _zipf(6 * 20000, 32).reshape(20000, 6)
    blob = np.concatenate([pairs.reshape(-1), _zipf((1 << 20) - 40000 * 14, 33)])
    ds = np.concatenate([np.arange(40001, dtype=np.uint64) * 14, [len(blob)]]).astype(np.uint64)
    return _Corpus(blob, ds)


@pytest.fixture(scope="module")
def long_corpus():
    # 2^22 bytes of Zipf-64 text in a few long documents and many short ones that are prefixes of each other (keys that end inside
    # the document: whole-suffix ties, final in the last pass), with a run of one symbol (one cell far larger than a tile)
    rng = np.random.default_rng(9)
    stems = _zipf(12 * 4000, 5).reshape(4000, 12)
    parts = [s[:k] for s in stems for k in rng.permutation(np.arange(1, 13))[:4]]
    body = _zipf((1 << 22) - sum(len(p) for p in parts), 6)
    body[1 << 20:(1 << 20) + 70000] = body[0]
    lens = [len(p) for p in parts] + [len(body) // 3, len(body) - len(body) // 3]
    ds = np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.uint64))]).astype(np.uint64)
    return _Corpus(np.concatenate(parts + [body]), ds)


def test_pair_corpus_on_and_off(capi, pair_corpus):
    g1, _ = pair_corpus.on_and_off(capi, **VL)
    assert g1.stat("carried_key_bits") == 5 and g1.stat("unresolved_after_initial") > 0


def test_long_corpus_on_and_off(capi, long_corpus):
    long_corpus.on_and_off(capi, **VL)


def test_several_bucket_groups(capi, pair_corpus):
    for frac in (0.55, 0.3):
        g1, _ = pair_corpus.on_and_off(capi, bucket_group_limit=int(len(pair_corpus.blob) * frac), **VL)
        assert g1.stat("bucket_groups") >= 2


@pytest.mark.parametrize("opts", [dict(carried_bits=0), dict(carried_bits=2), dict(pack_sa=0), dict(plain_tile_order=1),
                                  dict(carried_inplace=1), dict(group_sort=0)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_beside_other_options(capi, pair_corpus, opts):
    pair_corpus.on_and_off(capi, **dict(VL, **opts))


def test_automatic_starts_at_2_to_26(capi, pair_corpus):
    g = pair_corpus.build(capi, **VL)
    assert g.stat("top_first") == 0 and g.stat("vl_key_bits") == 40


def test_forms_it_does_not_apply_to(capi, pair_corpus):
    # dense keys (no sweep: no variable-length keys), other key widths (one or three low digits)
    g = pair_corpus.build(capi, top_digit_first=1, sweep_records=0, fuse_records=0, **VL)
    assert g.stat("vl_key_bits") == 0 and g.stat("top_first") == 0
    for bits in (32, 48):
        g = pair_corpus.build(capi, top_digit_first=1, force_big_path=1, vl_keys=bits)
        assert g.stat("top_first") == 0, bits
    for off in ("segmented_sort", "pack_entries"):      # (without packed entries the build takes no variable-length keys)
        g = pair_corpus.build(capi, top_digit_first=1, **dict(VL, **{off: 0}))
        assert g.stat("top_first") == 0, off


def test_rotated_bucket_under_variable_length_keys(capi):
    # Zipf-64 text whose symbols are 40 ASCII bytes and 24 bytes >= 0x80: few enough symbols for 40-bit variable-length keys, and in
    # the reference's order the buckets of a radix node are written rotated (depth-1 folds) — the form is asked for and must stay off
    z = _zipf(1 << 20, 41)
    sym = np.unique(z)
    table = np.zeros(256, dtype=np.uint8)
    table[sym] = np.concatenate([np.arange(0x30, 0x30 + 40), np.arange(0xC0, 0xC0 + 24)]).astype(np.uint8)[np.random.default_rng(3).permutation(len(sym))]
    blob = table[z]
    assert len(sym) == 64 and (blob >= 0x80).any() and (blob < 0x80).any()
    lens = np.full(40001, 14, dtype=np.uint64)                  # (16 document bits + 19 offset bits: 8-byte entries, as in pair_corpus)
    lens[13000] += len(blob) - 40001 * 14
    c = _Corpus(blob, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    g1 = c.build(capi, top_digit_first=1, **VL)
    g0 = c.build(capi, top_digit_first=0, **VL)
    assert g1.stat("vl_key_bits") == 40 and g1.stat("compat_rotations") > 0 and g1.stat("segmented") == 1
    assert g1.stat("top_first") == 0 and g0.stat("top_first") == 0
    for name in SAME + ("compat_rotations",):
        assert g1.stat(name) == g0.stat(name), name
    assert "rs_seg_k32_v32_w16_t16384" in g1.profile() and "rs_seg_top_w16_t16384" not in g1.profile()


def test_dense_keys_in_the_reference_order(capi):
    # UTF-8 text (more than 127 symbols: dense keys) built bucket-wise with rotated buckets: the form is not wanted at all
    blob, ds = W.utf8_corpus(4096, 256, seed=4)
    c = _Corpus(blob, ds)
    g1 = c.build(capi, top_digit_first=1, force_big_path=1)
    assert g1.stat("vl_key_bits") == 0 and g1.stat("compat_rotations") > 0 and g1.stat("top_first") == 0
