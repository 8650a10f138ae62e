"""The referee of tests/sweep_referee.py, pinned on the CPU: its slow per-position form equals its numpy form, both key forms
preserve the suffix order, every named case of tests/test_gpu_sweep_edges.py reaches the edge it is named for, and every case stays
inside the parameters the build can choose (Case.build runs check_domain)."""
import numpy as np
import pytest

from tests import sweep_referee as R

TILE, NT = R.TILE, R.NT


def _small(seed, sigma, n=700, mean=7, bits=None, empty=True):
    rng = np.random.default_rng(seed)
    ds = R.random_docs(rng, n, mean)
    if empty:                                                    # empty documents in the middle and at the end
        ds = np.sort(np.concatenate([ds, ds[[3, 3, len(ds) // 2]], [n]])).astype(np.uint64)
    return R.Corpus(R.random_text(rng, n, sigma, skew=True), ds, bits or R.bits_for(ds))


SMALL_PLANS = [("dense", (5, 4, 1)), ("dense", (5, 5, 3)), ("dense", (16, 11, 1)), ("dense", (40, 11, 1)), ("dense", (23, 11, 2)),
               ("vl", ("comb", 16, 5)), ("vl", ("two", 40, 6)), ("vl", ("seven", 56, 2)), ("vl", ("comb", 48, 0))]


def _plan(c, kind, args):
    if kind == "dense":
        return R.DensePlan(*args)
    return R.VlPlan(R.VL_CODES[args[0]](), args[1], args[2], R.entry_high_bits(c))


@pytest.mark.parametrize("kind,args", SMALL_PLANS, ids=str)
def test_slow_and_numpy_forms_agree(kind, args):
    sigma = {"comb": 6, "two": 2, "seven": 30}.get(args[0], min(args[0] - 1, 12) if kind == "dense" else 0)
    c = _small(11, sigma)
    plan = _plan(c, kind, args)
    R.check_domain(c, plan)
    rec = R.records(c, plan)
    for g0, g1 in [(0, c.sigma)] + R.even_groups(c, 3):
        g = R.group(rec, g0, g1)
        k, v, w = R.records_slow(c, plan, g0, g1, g["gstart"], rec["slot_start"])
        sl = slice(g["gstart"], g["gstart"] + g["gelems"])
        assert None not in k and k == rec["k"][sl].tolist() and v == rec["v"][sl].tolist() and w == rec["w"][sl].tolist()
        h = R.histogram(rec["k"][sl], rec["w"][sl], g["seg_begin"], g["seg_end"], plan.lead, plan.npass)
        assert np.array_equal(h, R.histogram_slow(k, w, g["seg_begin"], g["seg_end"], plan.lead, plan.npass))
        assert int(h[:, :plan.npass].sum()) == plan.npass * g["gelems"] and int(h[:, plan.npass:].sum()) == 0


def test_entries_above_32_bits_go_into_the_aux_word():
    rng = np.random.default_rng(3)
    n = 3000
    c = R.Corpus(R.random_text(rng, n, 6), np.array([0, 10, n], dtype=np.uint64), 22)    # offset 1024 << 22 = 2^32
    for plan in (R.DensePlan(16, 11), R.VlPlan(R.VL_CODES["comb"](), 40, 5, R.entry_high_bits(c))):
        R.check_domain(c, plan)
        rec = R.records(c, plan)
        k, v, w = R.records_slow(c, plan, 0, c.sigma, 0, rec["slot_start"])
        assert k == rec["k"].tolist() and v == rec["v"].tolist() and w == rec["w"].tolist()
        assert R.entry_high_bits(c) == 2 and {(x >> plan.low) & 3 for x in w} == {0, 1, 2}


def _suffix(c, p):
    """the suffix as the build orders it: its codes up to the end of its document (a shorter suffix first: END < every code)"""
    return tuple(c.codes[p:int(c.doc_end[p])].tolist())


@pytest.mark.parametrize("kind,args", SMALL_PLANS, ids=str)
def test_keys_preserve_the_suffix_order(kind, args):
    """(a): inside a bucket key(a) < key(b) implies suffix(a) < suffix(b), (key, carried) likewise, and equal FINAL keys mean
    equal suffixes — by brute force over all pairs"""
    sigma = {"comb": 6, "two": 2, "seven": 30}.get(args[0], min(args[0] - 1, 4) if kind == "dense" else 0)
    c = _small(5, sigma, n=420, mean=5 if kind == "dense" else 9)
    plan = _plan(c, kind, args)
    key, carried = R.keys(c, plan)
    finals = 0
    for s in range(c.sigma):
        ps = np.flatnonzero(c.slots == s).tolist()
        suf = {p: _suffix(c, p) for p in ps}
        for a in ps:
            ka, xa = int(key[a]), int(carried[a])
            for b in ps:
                kb, xb = int(key[b]), int(carried[b])
                if ka < kb or (ka == kb and xa < xb):
                    assert suf[a] < suf[b], (a, b, ka, kb, xa, xb)
                if ka == kb and a < b and plan.final(ka):
                    finals += 1
                    assert suf[a] == suf[b], (a, b, ka)
            if kind == "dense":                                  # final = the document ends inside the key's whole symbols
                assert plan.final(ka) == (len(suf[a]) - 1 < plan.nsym - 1), (a, ka)
    assert finals > 0                                            # (equal final keys occur at all: repeated short documents)


def test_open_suffix_count_is_the_flag_rule():
    """open_suffixes against a direct reading of sa_flags_of over the sorted (bucket, key) sequence"""
    c = _small(9, 4, n=3000, mean=6)
    for plan in (R.DensePlan(5, 4, 1), R.DensePlan(5, 4, 3), R.VlPlan(R.VL_CODES["comb"](), 16, 5, 0)):
        key, carried = R.keys(c, plan)
        for with_carried in (False, True):
            rows = sorted((int(s), int(k), int(x) if with_carried else 0) for s, k, x in zip(c.slots, key, carried))
            want = 0
            for i, r in enumerate(rows):
                head = i == 0 or rows[i - 1] != r
                tail = i + 1 == len(rows) or rows[i + 1] != r
                want += (not (head and tail)) and not plan.final(r[1])
            assert R.open_suffixes(c, plan, with_carried) == want
        assert R.open_suffixes(c, plan, True) <= R.open_suffixes(c, plan, False)


def test_code_tables_equal_the_library_s():
    """VlCode.tables against vl_fill_tables (cdb_debug_vl_tables, host only), and the production code is an alphabetic code"""
    from coffeedb_amd import capi
    for sigma in (2, 3, 17, 64, 127):
        counts = R.zipf_counts(sigma, 1 << 20, 1 << 10)
        slot_of_code = np.concatenate([[0], np.arange(sigma)]).astype(np.uint8)
        sym, dec, end_len = capi.debug_vl_tables(counts, slot_of_code)
        code = R.VlCode.from_tables(sym, sigma)                  # (the constructor asserts order and prefix-freedom)
        sym2, dec2 = code.tables(slot_of_code)
        assert np.array_equal(sym, sym2) and np.array_equal(dec, dec2) and end_len == code.end_len
        assert R.VlCode.from_lengths(code.length).word == code.word
    with pytest.raises(capi.SweepError):
        capi.debug_vl_tables(np.array([1, 5], dtype=np.uint64), np.array([0, 0], dtype=np.uint8))   # one symbol: no code


def test_tie_corpus_tells_weaker_keys_apart():
    """the corpus of the build test in tests/test_gpu_sweep_edges.py reaches what its count must see: the open suffixes change when
    the quantised symbol is not cut at the document end, when "continues" is set one bit early, and when a carried bit is lost"""
    from coffeedb_amd import capi
    blob, ds = R.tie_corpus()
    c = R.Corpus(blob, ds, 16)
    assert c.D == 36001 and c.sigma == 64 and capi.layout_rule(c.D, 300000)[0] == 16 and capi.layout_rule(c.D, 300000)[3] == 19
    pos = np.arange(c.n)
    left = c.doc_end - pos - 1
    # dense, key_symbols = 6 with three levels: documents end exactly behind the key's five whole symbols, in front of a live symbol
    plan = R.DensePlan(65, 6, 3)
    at = np.flatnonzero((left == 5) & (c.doc_end < c.n))
    assert len(at) > 1000 and np.count_nonzero(c.codes[c.doc_end[at]] * 3 // 65) > 100
    # variable-length: tied positions right at avail + end_len = key_bits - 1, and ties that part in the LAST carried bit only
    counts = np.concatenate([[c.D], c.byte_counts[c.byte_of_code[1:]]]).astype(np.uint64)
    sym, _, _ = capi.debug_vl_tables(counts, np.concatenate([[0], np.arange(c.sigma)]).astype(np.uint8))
    code = R.VlCode.from_tables(sym, c.sigma)
    open5, open4 = (R.open_suffixes(c, R.VlPlan(code, 40, x, 3), with_carried=True) for x in (5, 4))
    assert 0 < open5 < open4 < R.open_suffixes(c, R.VlPlan(code, 40, 5, 3))
    off = np.concatenate([[0], np.cumsum(np.array(code.length)[c.codes])])
    avail = off[c.doc_end] - off[pos + 1]
    key = R.vl_keys(c, R.VlPlan(code, 40, 0, 3))[0]
    edge = np.flatnonzero(avail + code.end_len == 39)
    assert len(edge) > 0 and all(int(k) & 1 == 0 for k in key[edge])
    _, cnt = np.unique(np.stack([c.slots[edge].astype(np.uint64), key[edge]]), axis=1, return_counts=True)
    assert (cnt >= 2).any()                                      # ... final and tied: one bit early they would count as open


# ---- (b) every named case reaches its edge ---------------------------------------------------------------------------------------
def _facts(case, g0=None, g1=None):
    b = case.build()
    return b, R.tile_facts(b["c"], b["plan"].vl, g0, g1)


@pytest.mark.parametrize("case", R.SHAPE_CASES, ids=repr)
def test_shape_cases_reach_their_edges(case):
    b, f = _facts(case)
    c, n = b["c"], b["reach"]["n"]
    assert c.n == n and n in R.SHAPE_SIZES and len(f) == -(-n // TILE)
    assert f[-1]["valid"] == (n - 1) % TILE + 1 and f[-1]["fast"] == (n % TILE == 0)
    if n >= 2 * TILE:
        assert f[0]["fast"] and f[0]["paired"] == (not b["plan"].vl)
        assert (c.text == 0x00).any() and (c.text == 0xA5).any()     # bytes that a read behind the text would fake
    assert b["reach"]["ragged"] == (n % 16 != 0)


def test_shape_sizes_are_the_named_ones():
    assert R.SHAPE_SIZES == [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 63, 2 * TILE + 64, 2 * TILE + 65]
    assert R.LOOK == 64 and {(vl, aux) for vl in R.KERNELS for aux in R.AUX} == {(c.build()["plan"].vl, c.build()["plan"].aux) for c in R.SHAPE_CASES}


@pytest.mark.parametrize("case", R.TILES_CASES, ids=repr)
def test_tiles_cases_reach_their_edges(case):
    b = case.build()
    r = b["reach"]
    assert r["tiles"] in (65, 129, 258) and r["tiles"] % R.GRID_GROUP != 0 and r["grid"] > r["tiles"]
    if r["tiles"] == 258:
        assert r["row_blocks"] == 2 and b["c"].n == 257 * TILE + 1 and r["rec_tiles"] > R.HIST_TILES
        assert b["groups"] == [(0, b["c"].sigma)]
    else:
        assert r["row_blocks"] == 1 and len(b["groups"]) == 2


@pytest.mark.parametrize("case", R.GROUPS_CASES, ids=repr)
def test_groups_cases_reach_their_edges(case):
    b, f = _facts(case, 0, 3)
    want = [0, 1, NT - 1, NT, NT + 1, 2 * NT - 1, 2 * NT, 2 * NT + 1]
    kept = [t["kept"] for t in f]
    assert kept[:len(R.KEPT_TARGETS)] == R.KEPT_TARGETS and all(x in kept for x in want) and TILE in kept
    assert any(NT < k % (2 * NT) <= NT + 16 and k > 2 * NT for k in kept)          # kept mod 2 NT just above NT: the round-5 shape
    assert all(t["fast"] for t in f)                                               # ... on the path that pairs or does not pair
    assert [t["paired"] for t in f].count(True) == (0 if b["plan"].vl else 1)
    assert (3, 4) in b["groups"] and (0, b["c"].sigma) in b["groups"] and len(b["groups"]) >= 4
    _, one = _facts(case, 3, 4)
    assert any(t["kept"] == 0 for t in one) and any(t["kept"] > 0 for t in one)    # a group absent from some tiles
    _, rest = _facts(case, 4, b["c"].sigma)
    assert sorted(t["kept"] for t in rest)[:2] == [0, 1]


@pytest.mark.parametrize("case", R.DOCUMENTS_CASES, ids=repr)
def test_documents_cases_reach_their_edges(case):
    b, f = _facts(case)
    c, edge = b["c"], b["reach"]["edge"]
    ds = c.doc_start.astype(np.int64)
    assert edge == (254 if b["plan"].vl else 182)
    assert [t["ndl"] for t in f[:3]] == [edge - 1, edge, edge + 1]
    assert [t["docs_in_lds"] for t in f[:3]] == [True, True, False] and [t["fast"] for t in f[:3]] == [True, True, False]
    assert 3 * TILE in ds and f[3]["fast"]                                          # rel == TILE for tile 2, rel == 0 for tile 3
    lens = np.diff(ds)
    assert np.count_nonzero(lens[(ds[:-1] >= 3 * TILE) & (ds[:-1] < 4 * TILE)] == 1) >= 39   # one-byte documents in a fast tile
    t4 = b["reach"]["empty_tile"]
    assert f[t4]["empty"] and f[t4]["docs_in_lds"] and not f[t4]["fast"] and f[t4]["valid"] == TILE
    assert [t["empty"] for t in f].count(True) == 1 + (1 if f[-1]["empty"] else 0)
    assert lens[-1] == 0 and ds[-2] == c.n                                          # an empty last document
    s, e = b["reach"]["long_doc"]
    assert s in ds and e in ds and e - s > 2 * TILE and s // TILE == 4 and e // TILE == 7     # one document over four tiles
    assert f[5]["fast"] and e - 5 * TILE > TILE + R.LOOK                            # ... beyond tile 5's look-ahead: the clamp
    assert f[6]["fast"] and TILE < e - 6 * TILE < TILE + R.LOOK                     # ... ending inside tile 6's look-ahead
    assert f[5]["ndl"] == 0 and f[6]["ndl"] == 0
    assert f[-1]["valid"] < TILE and not f[-1]["fast"]


@pytest.mark.parametrize("case", R.ENTRIES_CASES, ids=repr)
def test_entries_cases_reach_their_edges(case):
    b, f = _facts(case)
    c, e = b["c"], b["c"].entries()
    kind = b["reach"]["kind"]
    if kind == "cross":
        p = int(np.flatnonzero(e >= (1 << 32))[0])
        assert int(e[p - 1]) < (1 << 32) and p % TILE not in (0, TILE - 1) and f[p // TILE]["fast"] and c.doc[p] == c.doc[p - 1]
    elif kind == "bits1":
        assert c.bits == 1 and c.D == 2
    else:
        assert (1 << 39) <= int(e.max()) < (1 << 40) and R.entry_high_bits(c) == 8 and c.bits + int(np.diff(c.doc_start.astype(np.int64)).max()).bit_length() == 40


def _end_distances(c, f, fast):
    """symbols left behind the bucket symbol, over the positions of the tiles that take (fast) or do not take the LDS tables"""
    pos = np.arange(c.n)
    on = np.array([t["fast"] for t in f])[pos // TILE] == fast
    return set((c.doc_end - pos - 1)[on].tolist())


@pytest.mark.parametrize("case", R.DENSE_KEY_CASES, ids=repr)
def test_dense_key_cases_reach_their_edges(case):
    b, f = _facts(case)
    c, plan = b["c"], b["plan"]
    assert f[1]["fast"] and not f[0]["docs_in_lds"] and c.sigma == plan.base - 1
    for fast in (True, False):                                   # a document end at every distance 0 .. nsym + 1 behind a kept position
        assert set(range(plan.nsym + 2)) <= _end_distances(c, f, fast)
    key = R.dense_keys(c, plan)[0]
    assert int(key.max()) >= plan.range // 2 and int(key.max()) < plan.range


def test_dense_key_shapes_are_the_named_ones():
    shapes = R.DENSE_KEY_SHAPES
    assert {s[1] - 1 for s in shapes if s[2] == 1} == set(range(1, 11))
    assert {2, 3, 16, 206, 255} <= {s[0] for s in shapes}
    for ns1 in (3, 4, 7, 8):                                     # the quantised symbol as the last byte of a window or the first of the next
        assert any(s[1] - 1 == ns1 and s[2] > 1 for s in shapes)
    assert any(s[2] == 2 for s in shapes) and any(s[2] == s[0] - 1 for s in shapes)
    assert {R.DensePlan(*s).aux for s in shapes} == {1, 2, 4}


@pytest.mark.parametrize("case", R.VL_KEY_CASES, ids=repr)
def test_vl_key_cases_reach_their_edges(case):
    b, f = _facts(case)
    c, plan = b["c"], b["plan"]
    name = b["reach"]["code"]
    kb1 = plan.key_bits - 1
    assert f[1]["fast"] and not f[0]["docs_in_lds"]
    lens = np.array(plan.code.length)[c.codes]
    off = np.concatenate([[0], np.cumsum(lens)])
    pos = np.arange(c.n)
    avail = off[c.doc_end] - off[pos + 1]
    fast = np.array([t["fast"] for t in f])[pos // TILE]
    for on in (fast, ~fast):
        assert (avail[on] < kb1).any()                                            # a document end inside the key's bits
        if plan.carry and name != "seven":                                        # (7-bit words can step over them)
            assert ((avail[on] >= kb1) & (avail[on] < kb1 + plan.carry)).any()    # ... inside the carried bits
        if name in ("comb", "two"):                                               # (7-bit words step over two of the three)
            edge = set((avail[on] + plan.code.end_len - kb1).tolist()) & {-1, 0, 1}
            assert edge == {-1, 0, 1}                                             # the "continues" compare and one to either side
    local = off[pos] - off[pos // TILE * TILE]                                    # bit offset inside the tile's stream
    assert ((local % 32 == 0) & fast & (local > 0)).any()                         # the sh == 0 branch
    if name == "comb":                                                            # exactly 64 stream bits in the look-ahead of tile 0
        assert int(off[TILE + R.LOOK] - off[TILE]) == 64 and c.doc[TILE - 100] == c.doc[TILE + 100] and f[0]["valid"] == TILE
    assert plan.code.sigma >= c.sigma


def test_vl_key_shapes_are_the_named_ones():
    assert {s[0] for s in R.VL_KEY_SHAPES} == {"seven", "comb", "two", "zipf"}
    assert {16, 40, 56} <= {s[1] for s in R.VL_KEY_SHAPES} and {0, 1, 5, 6} <= {s[2] for s in R.VL_KEY_SHAPES}
    assert set(R.VL_CODES["seven"]().length) == {7} and 1 in R.VL_CODES["comb"]().length and R.VL_CODES["two"]().sigma == 2
    z = R.VL_CODES["zipf"]()
    assert z.sigma == 64 and min(z.length) < max(z.length) <= 7


@pytest.mark.parametrize("case", R.HIST_CASES, ids=repr)
def test_hist_cases_reach_their_edges(case):
    b = case.build()
    c, plan, rec = b["c"], b["plan"], b["rec"]
    sizes = rec["slot_count"].tolist()
    assert sizes == [1, 2, 3, 4, 5, R.SEG_TILE - 1, R.SEG_TILE, R.SEG_TILE + 1]
    g = R.group(rec, 0, c.sigma)
    assert {int(x) % 4 for x in g["seg_begin"]} == {0, 1, 2, 3}
    assert plan.lead == int(repr(case)[-1]) and plan.low == 8 * plan.lead
    assert g["seg_tile_begin"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and g["seg_tiles"] == 9


def test_every_case_is_listed_once_and_small():
    names = [repr(c) for c in R.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in R.ALL_CASES:
        b = c.build()
        assert b["c"].n <= 257 * TILE + 1
        for g0, g1 in b["groups"]:
            g = R.group(b["rec"], g0, g1)
            assert 0 <= g0 < g1 <= b["c"].sigma and g["gelems"] >= 1 and g["seg_tiles"] >= 1
            assert int(g["seg_end"][-1]) == g["gelems"]
