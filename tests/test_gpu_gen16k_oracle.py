"""Literal oracle parity for the 16 Ki-tile records generator of the radix pass (radix_pass.h: TextGenRec with 1024 threads).

With counted tile bases (option gen_prebased, the default) the generated pass of the fused bucket records runs as the 512-thread
look-back-free form; the 1024-thread instantiation runs only without the counts, and no other test of a few seconds asks for
that.  Here: gen_prebased = 0 on a text of 34 tiles of 16 Ki plus a ragged last one, documents of 1-24 bytes (so a thread's 16
consecutive positions hold document boundaries) and documents that end 1, 3 and 5 bytes in front of a tile end and exactly on one
(inside the key's nsym symbols: where the document lookup and the rolling window meet a tile edge).
(The 1024-thread TextGenPair instantiation has no such case: the MSD-first sort counts its tiles whenever it takes the pair form
— sa_build.hip: build prologue, msd_span — so the library never launches it.)

    cdb_sa_copy == oracle array (ties canonicalised), element for element          (index.h:66-73, index.cpp:86-126)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384


def _corpus(n_bytes, seed, long_doc=0):
    """text over 'a'..'p' (Zipf-like), documents of 1-24 bytes, optional one long document in the middle, document ends forced
    just in front of and on the first tile ends"""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, 17)
    blob = (0x61 + rng.choice(16, size=n_bytes, p=w / w.sum())).astype(np.uint8)
    cuts = np.cumsum(rng.integers(1, 25, size=n_bytes // 4))
    cuts = cuts[cuts < n_bytes]
    forced = np.array([TILE - 1, 2 * TILE - 3, 3 * TILE - 5, 4 * TILE], dtype=np.int64)
    forced = forced[forced < n_bytes]
    cuts = np.union1d(cuts, forced)
    if long_doc:
        a = n_bytes // 2
        cuts = cuts[(cuts <= a) | (cuts >= a + long_doc)]
    ds = np.concatenate([[0], cuts, [n_bytes]]).astype(np.uint64)
    ds = np.unique(ds)
    return blob, ds, forced


def _oracle_sa(blob, ds, ids):
    from oracle import OracleIndex
    o = OracleIndex()
    o.add_bulk(ids, blob, ds)
    o.build()
    o.canonicalize()
    return o.sa().copy(), (o.size, o.bits, o.mask, o.sa_width)


def _build_and_compare(blob, ds, opts, want_stats):
    from coffeedb_amd import capi
    ids = np.arange(len(ds) - 1, dtype=np.int64) * 3 + 1
    osa, meta = _oracle_sa(blob, ds, ids)
    g = capi.GpuStringIndex()
    try:
        for k, v in opts.items():
            g.set_option(k, v)
        g.add_bulk(ids, blob, ds)
        g.build()
        info = (opts, {k: g.stat(k) for k in ("bucketed", "msd_first", "key_layout", "key_symbols", "fused_records", "sweep_records",
                                             "gen_prebased", "self_check_fallbacks", "group_fallbacks", "dense_key_retries")})
        print(info)
        for k, v in want_stats.items():
            assert g.stat(k) == v, (k, info)
        assert g.stat("self_check_fallbacks") == 0 and g.stat("group_fallbacks") == 0, info  # (a fallback would mask a wrong array)
        assert (g.size, g.bits, g.mask, g.sa_width) == meta, info
        gsa = g.sa()
        assert gsa.dtype == osa.dtype and gsa.shape == osa.shape, info
        if not np.array_equal(gsa, osa):
            bad = np.flatnonzero(gsa != osa)
            raise AssertionError((info, "entries differ", int(bad.size), "first at", int(bad[0]), "last at", int(bad[-1])))
    finally:
        g.close()


def test_corpus_has_the_edges_it_is_built_for():
    blob, ds, forced = _corpus(5 * TILE + 777, seed=5)
    ends = set(int(x) for x in ds[1:])
    assert all(int(f) in ends for f in forced)                      # documents end 1, 3, 5 bytes in front of a tile end and on one
    assert int(np.diff(ds.astype(np.int64)).max()) <= 24            # a boundary inside (almost) every thread's 16 positions ...
    starts = np.asarray(ds[:-1], dtype=np.int64)
    per_thread = np.bincount(starts // 16, minlength=(5 * TILE + 777 + 15) // 16)
    assert (per_thread >= 1).mean() > 0.5 and per_thread.max() >= 3  # ... and several inside some


def test_records_generator_on_16k_tiles_equals_the_oracle():
    # bucket-wise build with fused records and 8-byte entries (one document of 2^17 bytes beside > 2^15 short ones: 33-bit
    # entries), dense keys, no counted tile bases: radix_gen_records launches RsBig + TextGenRec
    blob, ds, _ = _corpus(34 * TILE + 4321, seed=6, long_doc=(1 << 17) + 5)
    _build_and_compare(blob, ds, dict(force_big_path=1, gen_prebased=0, vl_keys=0, partial_symbol=0),
                       dict(bucketed=1, fused_records=1, sweep_records=0, gen_prebased=0, dense_key_retries=0))
