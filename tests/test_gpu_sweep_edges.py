"""The record sweeps of the bucket-wise build (records_sweep.h: rs_sweep_records_kernel, rs_sweep_records_vl_kernel) and the bucket
histograms counted from their records (rs_seg_hist_kernel) on their own, at the edges of their tiles, groups, documents, entries and
key shapes, run for one bucket group the way the build runs them (cdb_debug_sweep_records, debug_sweep.hip) and compared with the
referee of tests/sweep_referee.py.  tests/test_sweep_referee.py asserts on the CPU that every case reaches the edge it is named for.

Every comparison is integer equality of k, v, w and the histogram, and the poisoned guards around the record buffers must hold.
One test ties the hand-made plans to production: the open suffixes three small builds report are the ones the referee's keys
leave tied — a key that has grown weaker than specified changes that count, and nothing else in the suite."""
import numpy as np
import pytest

from tests import sweep_referee as R

pytestmark = pytest.mark.gpu

E_INVALID = 1


def _hook(c, plan, tables, g, padded, **over):
    from coffeedb_amd import capi
    args = dict(text=c.text, doc_start=c.doc_start, bits=c.bits, padded=padded, codeslot=tables["codeslot"], slotmap=tables["slotmap"],
                src_col=tables["src_col"], slot_start=tables["slot_start"], rec_low_bits=plan.low, aux_bytes=plan.aux, g0=g["g0"], g1=g["g1"],
                gstart=g["gstart"], gelems=g["gelems"], seg_begin=g["seg_begin"], seg_end=g["seg_end"], seg_tile_begin=g["seg_tile_begin"],
                lead=plan.lead, npass=plan.npass, tile_counts=tables["tile_counts"])
    args.update(plan.hook_args(c))
    args.update(over)
    return capi.debug_sweep_records(**args)


def _check(case, padded):
    b = case.build()
    c, plan, rec = b["c"], b["plan"], b["rec"]
    for g0, g1 in b["groups"]:
        g = R.group(rec, g0, g1)
        out = _hook(c, plan, b["tables"], g, padded)
        what = (repr(case), "padded" if padded else "unpadded", "group", g0, g1)
        assert out["guard_ok"], what
        sl = slice(g["gstart"], g["gstart"] + g["gelems"])
        for name in ("k", "v", "w"):
            bad = np.flatnonzero(out[name] != rec[name][sl])
            if len(bad):
                r = int(bad[0])
                p = int(rec["pos"][sl][r])                       # where the record comes from: position, tile, place in the tile
                assert False, (name, what, len(bad), "wrong records; first", r, "position", p, "tile", p // R.TILE, "at", p % R.TILE,
                               "document ends in", int(c.doc_end[p]) - p - 1, "got", hex(int(out[name][r])), "want", hex(int(rec[name][sl][r])),
                               "tile_base", out["tile_base"][p // R.TILE][int(c.slots[p])].item(), "tile_doc", out["tile_doc"][p // R.TILE].item())
        want = R.histogram(rec["k"][sl], rec["w"][sl], g["seg_begin"], g["seg_end"], plan.lead, plan.npass)
        bad = np.argwhere(out["hist"] != want)
        assert len(bad) == 0, ("histogram", what, "first wrong (segment, pass, digit)", bad[0].tolist(), int(out["hist"][tuple(bad[0])]), int(want[tuple(bad[0])]))


@pytest.mark.parametrize("padded", [0, 1])
@pytest.mark.parametrize("case", R.SHAPE_CASES, ids=repr)
def test_tile_shapes(case, padded):
    """n = 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 TILE, 2 TILE + 63 / 64 / 65 for both kernels and every aux width; an unpadded
    buffer whose n is no multiple of 16 takes the bytewise fetch; the text holds real 0x00 and 0xA5 bytes, so a byte faked behind
    the text would carry a live code"""
    _check(case, padded)


@pytest.mark.parametrize("case", R.TILES_CASES, ids=repr)
def test_many_tiles(case):
    """65 and 129 tiles (the XCD tile map, the grid rounded up to whole groups of 64 tiles), 257 tiles + 1 byte (two row blocks of
    rs_tile_bases; one group of more than 32 record tiles per bucket for the histogram sweep)"""
    _check(case, 1)


@pytest.mark.parametrize("case", R.GROUPS_CASES, ids=repr)
def test_groups_that_keep_chosen_parts_of_a_tile(case):
    """three uneven groups over tiles that keep 0, 1, NT - 1, NT, NT + 1, 2 NT - 1, 2 NT, 2 NT + 1, 3 NT + 7 (kept mod 2 NT just above
    NT) and all positions; a group of one bucket that is absent from every other tile; everything in one group (the paired loop)"""
    _check(case, 1)


@pytest.mark.parametrize("padded", [0, 1])
@pytest.mark.parametrize("case", R.DOCUMENTS_CASES, ids=repr)
def test_documents_at_the_edges_of_the_tile_tables(case, padded):
    """tiles with 181 / 182 / 183 (dense) and 253 / 254 / 255 (variable-length) document starts, a start on a tile's first position,
    one-byte documents, an empty document in an otherwise fast tile, one document over four tiles that ends inside a look-ahead,
    an empty last document, a ragged last tile"""
    _check(case, padded)


@pytest.mark.parametrize("case", R.ENTRIES_CASES, ids=repr)
def test_entries(case):
    """offsets that cross 2^32 inside a tile (the high bits go into w), bits = 1, and 25 + 15 = 40 entry bits"""
    _check(case, 1)


@pytest.mark.parametrize("case", R.DENSE_KEY_CASES, ids=repr)
def test_dense_key_shapes(case):
    """nsym - 1 = 1 .. 10, base = 2, 3, 16, 206, 255, the quantised next symbol at nsym - 1 = 3, 4, 7, 8 with part_m = 2 and base - 1;
    document ends at every distance behind a kept position, on the generic path (tile 0) and from the LDS tables (tile 1)"""
    _check(case, 1)


@pytest.mark.parametrize("case", R.VL_KEY_CASES, ids=repr)
def test_variable_length_key_shapes(case):
    """hand-written codes (all words 7 bits, a comb with a 1-bit word, two symbols) and the build's own code for Zipf counts;
    key_bits = 16, 40, 52, 56 and 0, 1, 2, 5, 6 carried bits; document ends inside the key, inside the carried bits and around
    avail + end_len = key_bits - 1; a run of the 1-bit word across the end of tile 0"""
    _check(case, 1)


@pytest.mark.parametrize("case", R.HIST_CASES, ids=repr)
def test_histograms_of_chosen_bucket_sizes(case):
    """buckets of 1, 2, 3, 4, 5, 16383, 16384 and 16385 records; group-local begins of every residue mod 4; lead = 0, 1, 2, 3"""
    _check(case, 1)


def test_hook_refuses_tables_that_are_not_the_text_s():
    """the sweeps trust their tables; the hook refuses what could send a record outside the group before it launches anything"""
    from coffeedb_amd import capi
    b = R.GROUPS_CASES[0].build()
    c, plan, t = b["c"], b["plan"], b["tables"]
    g = R.group(b["rec"], 0, 3)
    counts = t["tile_counts"].copy()
    counts[1, int(c.byte_of_code[1])] += 1
    start = t["slot_start"].copy()
    start[1] += 1
    short = dict(g, gelems=g["gelems"] - 1)
    for over in (dict(tile_counts=counts), dict(slot_start=start), dict(gelems=short["gelems"]), dict(lead=plan.npass + 1), dict(npass=9)):
        with pytest.raises(capi.SweepError) as e:
            _hook(c, plan, t, g, 1, **over)
        assert e.value.status == E_INVALID, over.keys()


# ---- the hand-made plans against production --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,opts", [("dense", dict(vl_keys=0, partial_symbol=0)), ("partial", dict(vl_keys=0, partial_symbol=1, key_symbols=6)),
                                       ("vl", dict(vl_keys=40))], ids=["dense", "partial", "vl"])
def test_open_suffixes_of_a_build_are_the_ties_of_the_referee_s_keys(form, opts):
    """A force_big_path build reports its key plan (alphabet, key_symbols, partial_levels, vl_key_bits, carried_key_bits) and how many
    suffixes its initial sort left open.  The referee rebuilds the keys from that plan (the code from cdb_debug_vl_tables) and counts
    the positions whose (bucket, key) class has two members or more and whose key is not final — sa_flags_of's rule; behind the
    carried round the same over (key, carried).  Refinement repairs any weaker key, so only this count can see one."""
    from coffeedb_amd import capi
    blob, ds = R.tie_corpus()
    g = capi.GpuStringIndex()
    for k, v in dict(opts, force_big_path=1).items():
        g.set_option(k, v)
    g.add_bulk(np.arange(len(ds) - 1, dtype=np.int64), blob, ds)
    g.build()
    assert g.stat("sweep_records") == 1 and g.stat("self_check_fallbacks") == 0 and g.stat("group_fallbacks") == 0
    c = R.Corpus(blob, ds, g.bits)
    assert g.stat("alphabet") == c.sigma
    if form == "vl":
        bits, _, _, off = capi.layout_rule(c.D, 300000)
        carry = int(g.stat("carried_key_bits"))
        assert g.stat("vl_key_bits") == 40 and bits + off == 35 and carry == min(40 - (bits + off), 6) == 5
        counts = np.concatenate([[c.D], c.byte_counts[c.byte_of_code[1:]]]).astype(np.uint64)
        sym, _, _ = capi.debug_vl_tables(counts, np.concatenate([[0], np.arange(c.sigma)]).astype(np.uint8))
        plan = R.VlPlan(R.VlCode.from_tables(sym, c.sigma), 40, carry, bits + off - 32)
    else:
        levels = int(g.stat("partial_levels"))
        assert g.stat("vl_key_bits") == 0 and (levels >= 2 if form == "partial" else levels == 0)
        plan = R.DensePlan(c.sigma + 1, int(g.stat("key_symbols")), max(levels, 1))
    want = R.open_suffixes(c, plan)
    assert want > 0 and g.stat("unresolved_after_initial") == want, (form, g.stat("unresolved_after_initial"), want)
    want_carried = R.open_suffixes(c, plan, with_carried=True) if form == "vl" else want
    assert g.stat("unresolved_after_carried") == want_carried, (form, g.stat("unresolved_after_carried"), want_carried)
    if form == "vl":
        assert want_carried < want
    g.close()
