"""CPU referee for the record sweeps of the bucket-wise build (coffeedb_amd/csrc/records_sweep.h) and the bucket histograms counted
from their records (radix_sort.h: rs_seg_hist_kernel), written from the header comments and the kernel text, in exact integers.

What the records ARE, independent of the finished suffix array:

  destination  every position p, in text order, whose bucket slot lies in [g0, g1) lands at
               slot_start[slot] - gstart + (number of earlier positions of that slot in the whole text);
  entry        e = (offset in document << bits) + document;  v = e mod 2^32;
  aux word     w = (key mod 2^low) | (e >> 32) << low | carried << carry_shift;   k = key >> low;
  dense key    the codes of the nsym - 1 symbols behind the bucket symbol as a number in base `base`, 0 from the document end on;
               with part_m > 1 that number x part_m + floor(code of the next symbol x part_m / base), same end rule;
  vl key       the code words behind the bucket symbol concatenated, zeros from the document end on: the first key_bits - 1 stream
               bits, then one bit (code bits left in the document + end_len > key_bits - 1); carried = the next `carry` stream bits;
  histogram    per segment, from the records: digit p < lead = byte p of w, digit lead + q = byte q of k.

Two forms of everything: a slow one per position in Python integers (`*_slow`) and a numpy one; tests/test_sweep_referee.py holds
them equal and pins that both key forms preserve the suffix order.  The named cases of tests/test_gpu_sweep_edges.py are built
here, each with the edge it is named for as data (`reach`), so that the CPU test can assert the edge is reached without a GPU."""
import bisect

import numpy as np

TILE, NT, LOOK = 8192, 512, 64
GRID_GROUP = 64            # tiles per grid group: 8 XCDs x RS_GROUP consecutive tiles
TB_ROWS, SEG_TILE = 256, 16384
HIST_TILES = 32            # record tiles per workgroup of the histogram sweep
DENSE_DOCS, VL_DOCS = 184, 256   # per-tile document tables of the two kernels (a tile with ndl + 2 <= DOCS starts uses them)
MAX_LEN = 7                # longest code word


# ---------------------------------------------------------------------------------------------------------------------------------
# corpus, tables, key plans
# ---------------------------------------------------------------------------------------------------------------------------------
class Corpus:
    """text, documents and the alphabet as the build derives it: symbol codes 1 .. sigma in byte order, bucket slot = code - 1."""

    def __init__(self, text, doc_start, bits):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        self.doc_start = np.ascontiguousarray(doc_start, dtype=np.uint64)
        self.n, self.D, self.bits = int(self.text.shape[0]), int(self.doc_start.shape[0]) - 1, int(bits)
        assert self.n >= 1 and self.D >= 1 and int(self.doc_start[0]) == 0 and int(self.doc_start[-1]) == self.n
        assert np.all(np.diff(self.doc_start.astype(np.int64)) >= 0)
        self.byte_counts = np.bincount(self.text, minlength=256).astype(np.uint64)
        present = np.flatnonzero(self.byte_counts)
        self.sigma = int(present.shape[0])
        self.code_of_byte = np.zeros(256, dtype=np.uint16)
        self.code_of_byte[present] = np.arange(1, self.sigma + 1, dtype=np.uint16)
        self.byte_of_code = np.concatenate([[0], present]).astype(np.int64)
        self.tiles = (self.n + TILE - 1) // TILE
        # document of every position: the largest d <= D - 1 with doc_start[d] <= p (rs_doc_upper), and where that document ends
        pos = np.arange(self.n, dtype=np.uint64)
        self.doc = (np.searchsorted(self.doc_start[:self.D], pos, side="right") - 1).astype(np.int64)
        self.doc_end = self.doc_start[self.doc + 1].astype(np.int64)
        self.codes = self.code_of_byte[self.text].astype(np.int64)
        self.slots = self.codes - 1

    def entries(self):
        pos = np.arange(self.n, dtype=np.uint64)
        return ((pos - self.doc_start[self.doc]) << np.uint64(self.bits)) + self.doc.astype(np.uint64)

    def entry_slow(self, p):
        ds = self.doc_start.tolist()
        d = bisect.bisect_right(ds, p, 0, self.D) - 1
        return ((p - ds[d]) << self.bits) + d

    def tables(self):
        """what the build uploads: codeslot, slotmap, src_col, slot_start, the per-tile byte counts"""
        slotmap = np.zeros(257, dtype=np.uint8)
        slotmap[1:self.sigma + 1] = np.arange(self.sigma, dtype=np.uint8)
        codeslot = (self.code_of_byte.astype(np.uint32) | (slotmap[self.code_of_byte].astype(np.uint32) << 8)).astype(np.uint16)
        src_col = np.full(256, 0xFFFF, dtype=np.uint16)
        src_col[:self.sigma] = self.byte_of_code[1:].astype(np.uint16)
        counts = self.byte_counts[self.byte_of_code[1:]]
        slot_start = np.full(256, self.n, dtype=np.uint64)
        slot_start[:self.sigma] = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        pad = np.full(self.tiles * TILE, -1, dtype=np.int64)
        pad[:self.n] = self.text
        tile_counts = np.stack([np.bincount(row[row >= 0], minlength=256) for row in pad.reshape(self.tiles, TILE)]).astype(np.uint32)
        return dict(codeslot=codeslot, slotmap=slotmap, src_col=src_col, slot_start=slot_start, tile_counts=tile_counts,
                    slot_count=counts.astype(np.uint64))


def record_shape(key_bits):
    """(rec_low_bits, aux_bytes) the build pairs with a key of that many bits (sa_build.hip: blow, auxb)"""
    assert 1 <= key_bits <= 56
    low = 0 if key_bits <= 32 else (8 if key_bits <= 40 else (16 if key_bits <= 48 else 24))
    return low, {0: 1, 8: 2, 16: 4, 24: 4}[low]


class DensePlan:
    def __init__(self, base, nsym, part_m=1):
        self.vl, self.base, self.nsym, self.part_m = False, int(base), int(nsym), int(part_m)
        self.range = self.base ** (self.nsym - 1) * self.part_m
        self.width = max(1, (self.range - 1).bit_length())
        self.low, self.aux = record_shape(self.width)
        self.carry = self.carry_shift = 0
        self.lead, self.npass = self.low // 8, (self.width + 7) // 8
        self.look = self.nsym - 1 + (1 if self.part_m > 1 else 0)   # symbols behind the bucket symbol that the key reads

    def final(self, key):
        return key % (self.base * self.part_m) == 0

    def hook_args(self, c):
        return dict(dense=(self.base, self.nsym, self.part_m))


class VlCode:
    """an alphabetic prefix code: word[c] / length[c] for c = 0 (END, all zeros) .. sigma"""

    def __init__(self, words, lengths):
        self.word, self.length = [int(x) for x in words], [int(x) for x in lengths]
        self.sigma, self.end_len = len(self.word) - 1, self.length[0]
        assert self.word[0] == 0 and all(1 <= l <= MAX_LEN and w < (1 << l) for w, l in zip(self.word, self.length))
        # in symbol order, prefix-free: left-aligned words ascend and no word is a prefix of the next
        al = [w << (MAX_LEN - l) for w, l in zip(self.word, self.length)]
        assert all(a + (1 << (MAX_LEN - l)) <= b for a, l, b in zip(al, self.length, al[1:]))

    @classmethod
    def from_lengths(cls, lengths):
        """the words of an alphabetic code with these depths: the next word is the previous one plus one, at the new length"""
        words, c = [], 0
        for i, l in enumerate(lengths):
            if i:
                c += 1
                c = c << (l - lengths[i - 1]) if l >= lengths[i - 1] else c >> (lengths[i - 1] - l)
            words.append(c)
        return cls(words, lengths)

    @classmethod
    def from_tables(cls, sym, sigma):
        return cls([int(sym[c]) & 0xFF for c in range(sigma + 1)], [int(sym[c]) >> 8 for c in range(sigma + 1)])

    def tables(self, slot_of_code):
        """the sweep's two tables (vl_code.h: vl_fill_tables)"""
        sym, dec = np.zeros(256, dtype=np.uint16), np.full(128, 0xFF | (self.end_len << 8), dtype=np.uint16)
        for c in range(self.sigma + 1):
            sym[c] = self.word[c] | (self.length[c] << 8)
            if c:
                lo = self.word[c] << (MAX_LEN - self.length[c])
                dec[lo:lo + (1 << (MAX_LEN - self.length[c]))] = int(slot_of_code[c]) | (self.length[c] << 8)
        return sym, dec


class VlPlan:
    def __init__(self, code, key_bits, carry, ehb):
        """ehb: bits of the entry above 32 (they sit in the aux word between the key's low bits and the carried bits)"""
        self.vl, self.code, self.key_bits, self.carry = True, code, int(key_bits), int(carry)
        self.width = self.key_bits
        self.low, self.aux = record_shape(self.key_bits)
        self.carry_shift = self.low + int(ehb)
        self.lead, self.npass = self.low // 8, (self.key_bits + 7) // 8

    def final(self, key):
        return key & 1 == 0

    def hook_args(self, c):
        sym, dec = self.code.tables([0] + list(range(self.code.sigma)))
        return dict(vl=(sym, dec, self.key_bits, self.code.end_len, self.carry, self.carry_shift))


def entry_high_bits(c):
    return max(0, int(c.entries().max()).bit_length() - 32)


def check_domain(c, plan):
    """(c) of the issue: the parameters stay inside what the build can choose"""
    assert c.bits >= 1 and int(c.entries().max()) < (1 << 40), "bits + offset bits <= 40"
    ehb = entry_high_bits(c)
    assert (plan.low, plan.aux) in ((0, 1), (8, 2), (16, 4), (24, 4))
    assert plan.low + ehb <= 8 * plan.aux
    if plan.vl:
        assert c.sigma <= 127 and plan.code.sigma >= max(2, c.sigma)
        assert 16 <= plan.key_bits <= 56 and plan.carry >= 0 and MAX_LEN + plan.key_bits - 1 + plan.carry <= 64
        assert plan.carry_shift >= plan.low + ehb and plan.carry_shift + plan.carry <= 8 * plan.aux
    else:
        assert 2 <= plan.base <= 255 and 1 <= plan.nsym - 1 <= 10 and c.sigma <= 254 and c.sigma < plan.base
        assert plan.range <= 1 << 56 and (plan.part_m == 1 or 2 <= plan.part_m <= plan.base - 1)
    assert plan.npass <= 8 and plan.lead <= plan.aux


# ---------------------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------------------
def dense_key_slow(c, plan, p):
    ds = c.doc_start.tolist()
    end = ds[bisect.bisect_right(ds, p, 0, c.D)]
    code = lambda q: int(c.code_of_byte[c.text[q]]) if q < end else 0
    key = 0
    for j in range(1, plan.nsym):
        key = key * plan.base + code(p + j)
    if plan.part_m > 1:
        key = key * plan.part_m + code(p + plan.nsym) * plan.part_m // plan.base
    return key


def dense_keys(c, plan):
    codes = np.concatenate([c.codes, np.zeros(16, dtype=np.int64)]).astype(np.uint64)
    pos = np.arange(c.n, dtype=np.int64)
    left = c.doc_end - pos - 1                       # symbols of the document behind the bucket symbol
    key = np.zeros(c.n, dtype=np.uint64)
    for j in range(1, plan.nsym):
        key = key * np.uint64(plan.base) + np.where(j <= left, codes[pos + j], np.uint64(0))
    if plan.part_m > 1:
        nxt = np.where(plan.nsym <= left, codes[pos + plan.nsym], np.uint64(0))
        key = key * np.uint64(plan.part_m) + nxt * np.uint64(plan.part_m) // np.uint64(plan.base)
    return key, np.zeros(c.n, dtype=np.uint64)


def vl_key_slow(c, plan, p):
    """(key, carried) from the document's own bytes, as a string of bits"""
    ds = c.doc_start.tolist()
    end = ds[bisect.bisect_right(ds, p, 0, c.D)]
    kb1, kbx = plan.key_bits - 1, plan.key_bits - 1 + plan.carry
    stream, q = "", p + 1
    while q < end and len(stream) <= kbx:           # (one bit more than the key reads decides "continues")
        cc = int(c.code_of_byte[c.text[q]])
        stream += format(plan.code.word[cc], "0%db" % plan.code.length[cc])
        q += 1
    cont = 1 if len(stream) + plan.code.end_len > kb1 else 0
    window = (stream + "0" * kbx)[:kbx]
    return (int(window[:kb1], 2) << 1) | cont, (int(window[kb1:], 2) if plan.carry else 0)


def vl_keys(c, plan):
    lens = np.array(plan.code.length, dtype=np.int64)[c.codes]
    words = np.array(plan.code.word, dtype=np.uint64)[c.codes]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)       # bit offset of every position's word in ONE stream
    nw = int(off[-1]) // 64 + 3
    stream = np.zeros(nw, dtype=np.uint64)
    room = 64 - (off[:-1] & 63) - lens                                   # >= 0: the word fits its 64-bit cell
    fits = room >= 0
    np.add.at(stream, off[:-1][fits] >> 6, words[fits] << room[fits].astype(np.uint64))
    over = (-room[~fits]).astype(np.uint64)                              # bits that spill into the next cell
    np.add.at(stream, off[:-1][~fits] >> 6, words[~fits] >> over)
    np.add.at(stream, (off[:-1][~fits] >> 6) + 1, (words[~fits] & ((np.uint64(1) << over) - np.uint64(1))) << (np.uint64(64) - over))
    pos = np.arange(c.n, dtype=np.int64)
    start = off[pos + 1]
    avail = off[c.doc_end] - start                                       # code bits between the bucket symbol and the document end
    wi, sh = start >> 6, (start & 63).astype(np.uint64)
    hi, lo = stream[wi], stream[wi + 1]
    top = np.where(sh == 0, hi, (hi << sh) | (lo >> ((np.uint64(64) - sh) & np.uint64(63))))
    kb1, kbx = plan.key_bits - 1, plan.key_bits - 1 + plan.carry
    take = np.minimum(avail, kbx).astype(np.uint64)
    win = (top >> np.uint64(64 - kbx)) & ~((np.uint64(1) << (np.uint64(kbx) - take)) - np.uint64(1))
    cont = (avail + plan.code.end_len > kb1).astype(np.uint64)
    key = ((win >> np.uint64(plan.carry)) << np.uint64(1)) | cont
    return key, win & ((np.uint64(1) << np.uint64(plan.carry)) - np.uint64(1))


def keys(c, plan):
    return vl_keys(c, plan) if plan.vl else dense_keys(c, plan)


def key_slow(c, plan, p):
    return vl_key_slow(c, plan, p) if plan.vl else (dense_key_slow(c, plan, p), 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# records, groups, histograms
# ---------------------------------------------------------------------------------------------------------------------------------
def records(c, plan, slot_start=None):
    """all records array-wide, in destination order: dict of pos (text position of every record), k, v, w, key, carried"""
    t = c.tables()
    slot_start = t["slot_start"] if slot_start is None else slot_start
    order = np.argsort(c.slots, kind="stable")                            # positions by (slot, text order)
    first = np.concatenate([[0], np.cumsum(t["slot_count"])[:-1]]).astype(np.int64)
    rank = np.arange(c.n, dtype=np.int64) - first[c.slots[order]]
    dest = (slot_start[c.slots[order]].astype(np.int64) + rank)
    assert np.array_equal(np.sort(dest), np.arange(c.n))                  # (the build's slot starts tile the array)
    pos = np.empty(c.n, dtype=np.int64)
    pos[dest] = order
    key, carried = keys(c, plan)
    e = c.entries()
    lowmask = np.uint64((1 << plan.low) - 1)
    w = (key & lowmask) | ((e >> np.uint64(32)) << np.uint64(plan.low)) | (carried << np.uint64(plan.carry_shift))
    assert int(w.max()) < (1 << (8 * plan.aux)) and int((key >> np.uint64(plan.low)).max()) < (1 << 32)
    wtype = {1: np.uint8, 2: np.uint16, 4: np.uint32}[plan.aux]
    return dict(pos=pos, k=(key >> np.uint64(plan.low)).astype(np.uint32)[pos], v=(e & np.uint64(0xFFFFFFFF)).astype(np.uint32)[pos],
                w=w.astype(wtype)[pos], key=key[pos], carried=carried[pos], slot_start=slot_start, slot_count=t["slot_count"])


def records_slow(c, plan, g0, g1, gstart, slot_start):
    """the group's records by the destination rule, one position at a time: lists k, v, w of gelems records (None = never written)"""
    gelems = sum(int(c.byte_counts[c.byte_of_code[s + 1]]) for s in range(g0, g1))
    k, v, w = [None] * gelems, [None] * gelems, [None] * gelems
    seen = [0] * 256
    for p in range(c.n):
        s = int(c.code_of_byte[c.text[p]]) - 1
        r = seen[s]
        seen[s] += 1
        if not g0 <= s < g1:
            continue
        key, carried = key_slow(c, plan, p)
        e = c.entry_slow(p)
        d = int(slot_start[s]) - gstart + r
        k[d], v[d] = key >> plan.low, e & 0xFFFFFFFF
        w[d] = (key & ((1 << plan.low) - 1)) | (e >> 32) << plan.low | carried << plan.carry_shift
    return k, v, w


def group(rec, g0, g1):
    """the hook's group arguments and the slice of the records: buckets [g0, g1) of records()"""
    st, cnt = rec["slot_start"].astype(np.int64), rec["slot_count"].astype(np.int64)
    gstart = int(st[g0])
    gelems = int(st[g1 - 1] + cnt[g1 - 1]) - gstart
    begin = st[g0:g1] - gstart
    end = begin + cnt[g0:g1]
    tiles = (cnt[g0:g1] + SEG_TILE - 1) // SEG_TILE
    tile_begin = np.concatenate([[0], np.cumsum(tiles)[:-1]])
    return dict(g0=g0, g1=g1, gstart=gstart, gelems=gelems, seg_begin=begin.astype(np.uint64), seg_end=end.astype(np.uint64),
                seg_tile_begin=tile_begin.astype(np.uint32), seg_tiles=int(tiles.sum()))


def histogram(k, w, seg_begin, seg_end, lead, npass):
    """[nseg][8][256] from the group's records"""
    hist = np.zeros((len(seg_begin), 8, 256), dtype=np.uint64)
    for i, (b, e) in enumerate(zip(seg_begin.tolist(), seg_end.tolist())):
        for p in range(npass):
            src, byte = (w, p) if p < lead else (k, p - lead)
            dig = (src[b:e].astype(np.uint64) >> np.uint64(8 * byte)) & np.uint64(0xFF)
            hist[i, p] = np.bincount(dig.astype(np.int64), minlength=256)
    return hist


def histogram_slow(k, w, seg_begin, seg_end, lead, npass):
    hist = np.zeros((len(seg_begin), 8, 256), dtype=np.uint64)
    for i, (b, e) in enumerate(zip(seg_begin.tolist(), seg_end.tolist())):
        for r in range(b, e):
            for p in range(npass):
                dig = (int(w[r]) >> (8 * p)) & 0xFF if p < lead else (int(k[r]) >> (8 * (p - lead))) & 0xFF
                hist[i, p, dig] += np.uint64(1)
    return hist


def open_suffixes(c, plan, with_carried=False):
    """positions whose (bucket, key[, carried]) class has two members or more and whose key is not final: what the build counts
    as unresolved behind the initial sort (sa_initial_direct.hip: sa_flags_of) and behind the carried round"""
    key, carried = keys(c, plan)
    cols = [carried, key, c.slots] if with_carried else [key, c.slots]
    order = np.lexsort(cols)
    same = np.ones(c.n - 1, dtype=bool)
    for col in cols:
        same &= col[order][1:] == col[order][:-1]
    tied = np.zeros(c.n, dtype=bool)
    tied[1:] |= same
    tied[:-1] |= same
    final = key % np.uint64(plan.base * plan.part_m) == 0 if not plan.vl else (key & np.uint64(1)) == 0
    return int(np.count_nonzero(tied & ~final[order]))


# ---------------------------------------------------------------------------------------------------------------------------------
# which path a tile takes (for the reach assertions: read off the kernels)
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_facts(c, vl, g0=None, g1=None):
    """per tile: valid, ndl (document starts behind the tile's first position up to the next tile's first), docs_in_lds, empty (an
    empty document among them: s_flag), fast (phase B from the LDS tables), kept"""
    ds = c.doc_start.astype(np.int64)
    docs = VL_DOCS if vl else DENSE_DOCS
    g0, g1 = (0, c.sigma) if g0 is None else (g0, g1)
    out = []
    for t in range(c.tiles):
        base = t * TILE
        valid = min(TILE, c.n - base)
        tdoc = lambda p: int(np.searchsorted(ds[:c.D], min(p, c.n - 1), side="right")) - 1
        dlo, dhi = tdoc(base), tdoc(base + TILE)
        ndl = dhi - dlo
        in_lds = ndl + 2 <= docs
        rel = ds[dlo + 1:dlo + ndl + 2] - base
        rel = rel[rel <= TILE]
        empty = bool(len(np.unique(rel)) != len(rel))
        s = c.slots[base:base + valid]
        kept = int(np.count_nonzero((s >= g0) & (s < g1)))
        out.append(dict(valid=valid, ndl=ndl, docs_in_lds=in_lds, empty=empty, fast=in_lds and not empty and valid == TILE, kept=kept,
                        paired=in_lds and not empty and valid == TILE and kept == TILE and not vl))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# corpora of the named cases
# ---------------------------------------------------------------------------------------------------------------------------------
def alphabet_bytes(sigma):
    """sigma byte values in ascending order, 0x00 and 0xA5 among them: a byte read as 0 behind the text, or the 0xA5 of a padded
    buffer, carries a live code"""
    rest = [b for b in range(255, 0, -1) if b != 0xA5]
    return np.array(sorted(([0x00, 0xA5] + rest)[:sigma]) if sigma >= 2 else [0x00], dtype=np.uint8)


def random_text(rng, n, sigma, skew=False):
    ab = alphabet_bytes(sigma)
    if skew:
        p = 1.0 / np.arange(1, sigma + 1)
        t = ab[rng.choice(sigma, size=n, p=p / p.sum())]
    else:
        t = ab[rng.integers(0, sigma, size=n)]
    t[:min(n, sigma)] = ab[:min(n, sigma)][rng.permutation(min(n, sigma))]     # every symbol occurs when the text is long enough
    return t


def random_docs(rng, n, mean):
    """document starts with lengths around `mean` (none empty)"""
    starts, p = [0], 0
    while True:
        p += int(rng.integers(1, 2 * mean))
        if p >= n:
            break
        starts.append(p)
    return np.array(starts + [n], dtype=np.uint64)


def mixed_docs(rng, n, short, long=64):
    """short documents in tile 0 (more starts than a tile's table holds: the generic path), documents around `long` bytes behind it
    (the LDS tables): a document end at every small distance behind a kept position on both paths"""
    a, b = random_docs(rng, TILE, short), random_docs(rng, n - TILE, long)
    return np.concatenate([a[:-1], b + np.uint64(TILE)]).astype(np.uint64)


def bits_for(doc_start):
    """the narrowest document field: bit_width(documents), at least 1"""
    return max(1, (len(doc_start) - 1).bit_length())


def even_groups(c, parts):
    """bucket groups of about equal numbers of slots"""
    cut = [round(i * c.sigma / parts) for i in range(parts + 1)]
    return [(a, b) for a, b in zip(cut, cut[1:]) if b > a]


class Case:
    """one hook input with everything the GPU test compares against; built lazily, once"""

    def __init__(self, name, make):
        self.name, self._make, self._built = name, make, None

    def build(self):
        if self._built is None:
            c, plan, groups, reach = self._make()
            check_domain(c, plan)
            self._built = dict(c=c, plan=plan, groups=groups, reach=reach, rec=records(c, plan), tables=c.tables())
        return self._built

    def __repr__(self):
        return self.name


# plans of every aux width for both kernels: (label, plan maker given the corpus)
DENSE_PLANS = {1: (16, 9, 1), 2: (16, 11, 1), 4: (40, 11, 1)}      # aux bytes -> (base, nsym, part_m): 32, 40 and 54 key bits
VL_PLANS = {1: (16, 5), 2: (40, 6), 4: (56, 2)}                     # aux bytes -> (key_bits, carry)
COMB = [6, 6, 5, 4, 3, 2, 1]                                        # END, then six symbols, the last with the 1-bit word "1"
SHAPE_SIZES = [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 63, 2 * TILE + 64, 2 * TILE + 65]


def dense_plan_for(c, aux):
    base, nsym, part_m = DENSE_PLANS[aux]
    return DensePlan(max(base, c.sigma + 1), nsym, part_m)


def vl_plan_for(c, aux, code=None, key_bits=None, carry=None):
    kb, cx = VL_PLANS[aux]
    kb, cx = (kb if key_bits is None else key_bits), (cx if carry is None else carry)
    code = code or VlCode.from_lengths([MAX_LEN] * (max(2, c.sigma) + 1))
    ehb = entry_high_bits(c)
    return VlPlan(code, kb, min(cx, 8 - ehb), ehb)       # (the build's cap: carried bits and the entry's high bits share one byte)


def plan_for(c, vl, aux, **kw):
    return vl_plan_for(c, aux, **kw) if vl else dense_plan_for(c, aux)


def shape_case(vl, aux, n, seed=1):
    """tile shapes: n around one thread's 16 bytes, one tile, the look-ahead; real 0x00 and 0xA5 bytes in the text"""
    def make():
        rng = np.random.default_rng(1000 * seed + n)
        sigma = 6 if vl else 15
        text = random_text(rng, n, sigma)
        ds = random_docs(rng, n, 120) if n > 1 else np.array([0, 1], dtype=np.uint64)
        c = Corpus(text, ds, bits_for(ds))
        plan = plan_for(c, vl, aux, code=VlCode.from_lengths(COMB)) if vl else plan_for(c, vl, aux)
        return c, plan, [(0, c.sigma)], dict(n=n, zero_byte=bool((text == 0).any()), ragged=n % 16 != 0)
    return Case("shape-%s-w%d-n%d" % ("vl" if vl else "dense", aux, n), make)


def tiles_case(vl, aux, tiles, extra, seed=2):
    """65 / 129 tiles (the XCD tile map, the grid rounded to whole groups) and 257 tiles + 1 (two row blocks of rs_tile_bases, more
    than 32 record tiles in one group); few symbols so that buckets span many record tiles"""
    def make():
        rng = np.random.default_rng(seed + tiles)
        n = tiles * TILE + extra
        sigma = 5
        text = random_text(rng, n, sigma, skew=True)
        ds = random_docs(rng, n, 300)
        c = Corpus(text, ds, bits_for(ds))
        plan = plan_for(c, vl, aux)
        groups = [(0, c.sigma)] if tiles > 200 else even_groups(c, 2)
        rec_tiles = max(int(np.sum((c.tables()["slot_count"][a:b].astype(np.int64) + SEG_TILE - 1) // SEG_TILE)) for a, b in groups)
        return c, plan, groups, dict(tiles=c.tiles, row_blocks=(c.tiles + TB_ROWS - 1) // TB_ROWS, grid=-(-c.tiles // GRID_GROUP) * GRID_GROUP,
                                     rec_tiles=rec_tiles)
    return Case("tiles-%s-w%d-%d+%d" % ("vl" if vl else "dense", aux, tiles, extra), make)


KEPT_TARGETS = [0, 1, NT - 1, NT, NT + 1, 2 * NT - 1, 2 * NT, 2 * NT + 1, 3 * NT + 7, 5 * NT + 1, TILE - 1, TILE]


def groups_case(vl, aux, seed=3):
    """three uneven bucket groups over tiles composed so that group A keeps exactly KEPT_TARGETS[t] positions of tile t (and group
    B + C the rest): kept = 0, 1, NT - 1 .. 2 NT + 1, kept mod 2 NT just above NT, everything; a group of one bucket; a group
    whose buckets are absent from a tile"""
    def make():
        rng = np.random.default_rng(seed)
        sigma = 9
        ab = alphabet_bytes(sigma)
        a_syms, b_syms, c_syms = ab[:3], ab[3:4], ab[4:]
        tiles = len(KEPT_TARGETS) + 1
        text = np.empty(tiles * TILE, dtype=np.uint8)
        for t in range(tiles):
            k = KEPT_TARGETS[t] if t < len(KEPT_TARGETS) else 3000
            row = np.empty(TILE, dtype=np.uint8)
            where = rng.permutation(TILE)
            row[where[:k]] = a_syms[rng.integers(0, 3, size=k)]
            rest = TILE - k
            nb = rest // 3 if t % 2 == 0 else 0               # (odd tiles: the one-bucket group B is absent)
            row[where[k:k + nb]] = b_syms[0]
            row[where[k + nb:]] = c_syms[rng.integers(0, len(c_syms), size=rest - nb)]
            text[t * TILE:(t + 1) * TILE] = row
        assert len(np.unique(text)) == sigma
        ds = random_docs(rng, len(text), 120)
        c = Corpus(text, ds, bits_for(ds))
        plan = plan_for(c, vl, aux)
        groups = [(0, 3), (3, 4), (4, sigma), (0, 4), (0, sigma)]
        return c, plan, groups, dict(kept_a=KEPT_TARGETS)
    return Case("groups-%s-w%d" % ("vl" if vl else "dense", aux), make)


def documents_case(vl, aux, seed=4):
    """documents at the edges of the per-tile tables: see the reach entries"""
    def make():
        rng = np.random.default_rng(seed)
        edge = (VL_DOCS if vl else DENSE_DOCS) - 2              # the most starts a tile's table takes
        n = 8 * TILE - 77
        starts = {0}

        def spread(t, count, lo=1, hi=TILE):
            """`count` distinct starts in (base, base + hi] of tile t"""
            starts.update((t * TILE + lo + rng.choice(hi - lo + 1, size=count, replace=False)).tolist())

        spread(0, edge - 1)
        spread(1, edge)
        spread(2, edge, hi=TILE - 1)
        starts.add(3 * TILE)                                     # rel == TILE for tile 2 (its start number edge + 1), rel == 0 for tile 3
        starts.update(range(3 * TILE + 100, 3 * TILE + 140))     # one-byte documents
        spread(3, 30, lo=200)
        tile4 = sorted((4 * TILE + 1 + rng.choice(4000, size=20, replace=False)).tolist())
        starts.update(tile4)
        starts.add(4 * TILE + 5000)                              # ... then one document over tiles 4 - 7: it ends inside the look-ahead of tile 6
        starts.add(7 * TILE + 30)
        starts.update((7 * TILE + 31 + rng.choice(TILE - 200, size=40, replace=False)).tolist())
        ds = sorted(starts)
        ds.insert(ds.index(tile4[7]), tile4[7])                  # an empty document inside tile 4
        ds = np.array(ds + [n, n], dtype=np.uint64)              # an empty last document
        sigma = 6 if vl else 15
        text = random_text(rng, n, sigma)
        c = Corpus(text, ds, bits_for(ds))
        plan = plan_for(c, vl, aux, code=VlCode.from_lengths(COMB)) if vl else plan_for(c, vl, aux)
        return c, plan, [(0, c.sigma)] + even_groups(c, 3), dict(edge=edge, empty_tile=4, long_doc=(4 * TILE + 5000, 7 * TILE + 30))
    return Case("documents-%s-w%d" % ("vl" if vl else "dense", aux), make)


def entries_case(vl, aux, kind):
    """entries: offsets that cross 2^32 inside a tile (the high bits go into w), bits = 1, the widest layout of 40 bits"""
    def make():
        rng = np.random.default_rng(50 + aux)
        n = 3 * TILE + 100
        if kind == "cross":
            ds, bits = np.array([0, 100, n], dtype=np.uint64), 18      # offset 16384 << 18 = 2^32 at position 16484, inside tile 2
        elif kind == "bits1":
            ds, bits = np.array([0, n - 5000, n], dtype=np.uint64), 1
        else:
            ds = random_docs(rng, n, 50)
            ds = np.unique(np.concatenate([ds, [TILE + 7, 3 * TILE + 50]])).astype(np.uint64)   # one document of 2 TILE + 43 < 2^15 bytes
            ds = ds[(ds <= TILE + 7) | (ds >= 3 * TILE + 50)]
            bits = 25                                                  # 15 offset bits + 25 = 40
        sigma = 6 if vl else 15
        c = Corpus(random_text(rng, n, sigma), ds, bits)
        plan = plan_for(c, vl, aux)
        return c, plan, [(0, c.sigma)], dict(kind=kind)
    return Case("entries-%s-w%d-%s" % ("vl" if vl else "dense", aux, kind), make)


DENSE_KEY_SHAPES = ([(16 if ns1 < 10 else 13, ns1 + 1, 1) for ns1 in range(1, 11)] +
                    [(2, 11, 1), (3, 8, 1), (206, 8, 1), (255, 8, 1), (255, 2, 1), (2, 2, 1)] +
                    [(b, ns1 + 1, m) for ns1 in (3, 4, 7, 8) for b, m in ((16, 2), (16, 15), (3, 2))] +
                    [(206, 6, 2), (206, 6, 205), (255, 5, 254), (255, 4, 2)])


def dense_key_case(base, nsym, part_m, seed=6):
    """dense key shapes: every nsym - 1, bases from 2 to 255, part_m off and on; short documents so that ends fall at every
    distance behind a kept position"""
    def make():
        rng = np.random.default_rng(seed + base * 100 + nsym)
        n = 2 * TILE + 300
        sigma = base - 1
        text = random_text(rng, n, sigma)
        ds = mixed_docs(rng, n, 9)
        c = Corpus(text, ds, bits_for(ds))
        return c, DensePlan(base, nsym, part_m), [(0, c.sigma)] + (even_groups(c, 2) if c.sigma > 1 else []), dict()
    return Case("densekey-b%d-n%d-m%d" % (base, nsym, part_m), make)


def production_code(sigma=64, n=1 << 20, docs=1 << 12):
    """the code the build would choose for a Zipf text (vl_build + vl_fill_tables through cdb_debug_vl_tables, host only)"""
    from coffeedb_amd import capi
    sym, _, end_len = capi.debug_vl_tables(zipf_counts(sigma, n, docs), np.concatenate([[0], np.arange(sigma)]).astype(np.uint8))
    code = VlCode.from_tables(sym, sigma)
    assert code.end_len == end_len
    return code


VL_CODES = {"seven": lambda: VlCode.from_lengths([MAX_LEN] * 101), "comb": lambda: VlCode.from_lengths(COMB),
            "two": lambda: VlCode.from_lengths([2, 2, 1]), "zipf": production_code}
VL_KEY_SHAPES = [(code, kb, cx) for code in ("seven", "comb", "two", "zipf") for kb, cx in ((16, 0), (16, 5), (40, 6), (40, 1), (56, 2), (56, 0), (52, 5))]


def vl_key_case(code_name, key_bits, carry, seed=7):
    """variable-length key shapes on hand-written codes; short documents: ends inside the key, inside the carried bits, at
    avail + end_len = key_bits - 1 and one to either side"""
    def make():
        rng = np.random.default_rng(seed + key_bits + carry)
        code = VL_CODES[code_name]()
        n = 2 * TILE + 300
        text = random_text(rng, n, code.sigma, skew=code_name in ("comb", "zipf"))
        if code_name == "comb":                                       # a run of the 1-bit symbol across the end of tile 0
            text[TILE - 200:TILE + 200] = alphabet_bytes(6)[5]
        mean = {"seven": 6, "comb": 14, "two": 20, "zipf": 8}[code_name] * max(1, key_bits // 16)
        ds = mixed_docs(rng, n, min(mean, 24), max(mean, 40))
        if code_name == "comb":
            ds = ds[(ds <= TILE - 300) | (ds >= TILE + 300)]           # ... inside one document
        c = Corpus(text, ds, bits_for(ds))
        return c, VlPlan(code, key_bits, carry, entry_high_bits(c)), [(0, c.sigma)] + even_groups(c, 2), dict(code=code_name)
    return Case("vlkey-%s-b%d-x%d" % (code_name, key_bits, carry), make)


def zipf_counts(sigma, n, docs):
    p = 1.0 / np.arange(1, sigma + 1)
    return np.concatenate([[docs], np.maximum(1, (n * p / p.sum())).astype(np.uint64)]).astype(np.uint64)


def hist_case(vl, lead_bytes, seed=8):
    """bucket sizes 1, 2, 3, 4, 5, 16383, 16384, 16385 in slot order: group-local begins 0, 1, 3, 6, 10, 15, 16398, 32782 — every
    residue mod 4 — and one record tile, a full one, a full one and one record; lead = lead_bytes low digits in the aux word"""
    def make():
        rng = np.random.default_rng(seed)
        sizes = [1, 2, 3, 4, 5, SEG_TILE - 1, SEG_TILE, SEG_TILE + 1]
        ab = alphabet_bytes(len(sizes))
        text = np.repeat(ab, sizes)
        rng.shuffle(text)
        ds = random_docs(rng, len(text), 60)
        c = Corpus(text, ds, bits_for(ds))
        if vl:
            plan = VlPlan(VlCode.from_lengths([4, 4, 4, 4, 3, 3, 3, 3, 3]), {0: 24, 1: 40, 2: 48, 3: 56}[lead_bytes], 0, entry_high_bits(c))
        else:
            plan = DensePlan({0: 9, 1: 13, 2: 23, 3: 40}[lead_bytes], 8 if lead_bytes == 0 else 11, 1)
        assert plan.lead == lead_bytes
        return c, plan, [(0, c.sigma), (1, 5), (2, 7), (5, 8), (3, 4)], dict(sizes=sizes)
    return Case("hist-%s-lead%d" % ("vl" if vl else "dense", lead_bytes), make)


KERNELS = (False, True)     # dense, variable-length
AUX = (1, 2, 4)

SHAPE_CASES = [shape_case(vl, aux, n) for vl in KERNELS for aux in AUX for n in SHAPE_SIZES]
TILES_CASES = ([tiles_case(vl, aux, 65, 0) for vl in KERNELS for aux in AUX] + [tiles_case(vl, 2, 129, 0) for vl in KERNELS] +
               [tiles_case(vl, 4 if vl else 1, 257, 1) for vl in KERNELS])
GROUPS_CASES = [groups_case(vl, aux) for vl in KERNELS for aux in AUX]
DOCUMENTS_CASES = [documents_case(vl, aux) for vl in KERNELS for aux in AUX]
ENTRIES_CASES = [entries_case(vl, aux, kind) for vl in KERNELS for aux in AUX for kind in ("cross", "bits1", "widest")]
DENSE_KEY_CASES = [dense_key_case(*s) for s in DENSE_KEY_SHAPES]
VL_KEY_CASES = [vl_key_case(*s) for s in VL_KEY_SHAPES]
HIST_CASES = [hist_case(vl, lead) for vl in KERNELS for lead in (0, 1, 2, 3)]
ALL_CASES = SHAPE_CASES + TILES_CASES + GROUPS_CASES + DOCUMENTS_CASES + ENTRIES_CASES + DENSE_KEY_CASES + VL_KEY_CASES + HIST_CASES


def tie_corpus(seed=77, sigma=64):
    """(text, doc_start) of the builds that tie the hand-made plans to production: pairs of 14-symbol documents that share their
    first eight symbols (about 41 code bits: ties that part inside the carried bits, bit by bit), documents of 1 .. 12 symbols, each
    of them twice (a document end at every distance behind a position; equal suffixes, so final keys that tie), and one document of 300 000 symbols
    with a repeat (ties no key resolves).  36 001 documents, the longest 300 000: 16 + 19 entry bits, room for 5 carried bits."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, sigma + 1)
    draw = lambda k: (0x30 + rng.choice(sigma, size=k, p=p / p.sum())).astype(np.uint8)
    pairs = np.repeat(draw(14 * 12000).reshape(12000, 14), 2, axis=0)
    pairs[1::2, 8:] = draw(6 * 12000).reshape(12000, 6)
    long_doc = draw(300000)
    long_doc[200000:260000] = long_doc[:60000]
    short_lens = np.repeat(np.tile(np.arange(1, 13), 500), 2)     # (every short document twice: equal suffixes, final keys that tie)
    short = [draw(int(k)) for k in short_lens[::2]]
    parts = [pairs.reshape(-1), long_doc] + [d for d in short for _ in range(2)]
    lens = np.concatenate([np.full(24000, 14), [300000], short_lens]).astype(np.uint64)
    return np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
