"""CPU referee for the segmented sort of bucket records with 40-bit variable-length keys (radix_sort.h: radix_sort_segmented over
five passes, radix_sort_top_first), stated twice: with Python integers (referee) and with numpy (referee_numpy).

Input: records in bucket order — bucket_begin[nb + 1], and per record a 40-bit key, an entry of at most 40 bits and its carried
bits.  Output: the entries in stable (bucket, key) order and one flag byte per slot: bit 0 = first of a group of equal keys of one
bucket, bit 1 = open — the slot belongs to a group of several and its key does not end inside the document, which a variable-length
key says in its lowest bit (clear = ends inside: sa_initial_direct.hip, sa_flags_of) — and the carried bits in bits 2 and up.
cells() is the cell table of the top-digit-first form: the non-empty (bucket, key >> 32) cells in order as (begin, end, tile_begin).
"""
import numpy as np

TILE = 16384


def referee(bucket_begin, key, entry, carried):
    n = len(key)
    order = []
    for b in range(len(bucket_begin) - 1):
        lo, hi = int(bucket_begin[b]), int(bucket_begin[b + 1])
        order += sorted(range(lo, hi), key=lambda i: (int(key[i]), i))
    bucket_of = [0] * n
    for b in range(len(bucket_begin) - 1):
        for i in range(int(bucket_begin[b]), int(bucket_begin[b + 1])):
            bucket_of[i] = b
    entries, flags = [], []
    for r, i in enumerate(order):
        same = lambda j: bucket_of[j] == bucket_of[i] and int(key[j]) == int(key[i])
        head = r == 0 or not same(order[r - 1])
        tail = r == n - 1 or not same(order[r + 1])
        f = 1 if head else 0
        if not (head and tail) and int(key[i]) & 1:
            f |= 2
        entries.append(int(entry[i]))
        flags.append(f | int(carried[i]) << 2)
    return entries, flags


def referee_numpy(bucket_begin, key, entry, carried):
    bb = np.asarray(bucket_begin, dtype=np.int64)
    key = np.asarray(key, dtype=np.uint64)
    n = len(key)
    bucket = np.repeat(np.arange(len(bb) - 1), np.diff(bb))
    order = np.lexsort((np.arange(n), key, bucket))
    k, b = key[order], bucket[order]
    differs = np.ones(n + 1, dtype=bool)
    differs[1:n] = (k[1:] != k[:-1]) | (b[1:] != b[:-1])
    head, tail = differs[:n], differs[1:]
    flags = head.astype(np.uint8)
    flags[~(head & tail) & ((k & np.uint64(1)) != 0)] |= 2
    flags |= (np.asarray(carried, dtype=np.uint8)[order] << 2).astype(np.uint8)
    return np.asarray(entry, dtype=np.uint64)[order], flags


def cells(bucket_begin, key):
    """(begin, end, tile_begin) of every non-empty (bucket, top byte) cell, in order"""
    out, tiles = [], 0
    for b in range(len(bucket_begin) - 1):
        lo, hi = int(bucket_begin[b]), int(bucket_begin[b + 1])
        tops = np.bincount((np.asarray(key[lo:hi], dtype=np.uint64) >> np.uint64(32)).astype(np.int64), minlength=256)
        at = lo
        for c in tops:
            if c:
                out.append((at, at + int(c), tiles))
                tiles += -(-int(c) // TILE)
                at += int(c)
    return np.array(out, dtype=np.uint64).reshape(-1, 3)


def split(form_top_first, key, entry, carried, ehb):
    """the records as the sweep writes them for the form: (k32, v32, w16)"""
    key = np.asarray(key, dtype=np.uint64)
    entry = np.asarray(entry, dtype=np.uint64)
    hi = (entry >> np.uint64(32)) | (np.asarray(carried, dtype=np.uint64) << np.uint64(ehb))
    if form_top_first:
        k32, low = key & np.uint64(0xFFFFFFFF), key >> np.uint64(32)
    else:
        k32, low = key >> np.uint64(8), key & np.uint64(0xFF)
    return k32.astype(np.uint32), (entry & np.uint64(0xFFFFFFFF)).astype(np.uint32), (low | hi << np.uint64(8)).astype(np.uint16)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, buckets, ehb=3, carry=5, seed=0):
        """buckets: per bucket a list of (top byte, low keys array) cells in any order; records are shuffled inside the bucket"""
        rng = np.random.default_rng(1000 + seed)
        self.name, self.ehb, self.carry = name, ehb, carry
        keys, bb = [], [0]
        for cs in buckets:
            k = [np.uint64(t) << np.uint64(32) | np.asarray(low, dtype=np.uint64) for t, low in cs]
            k = np.concatenate(k) if k else np.zeros(0, dtype=np.uint64)
            keys.append(rng.permutation(k))
            bb.append(bb[-1] + len(k))
        self.key = np.concatenate(keys)
        self.bucket_begin = np.array(bb, dtype=np.uint64)
        n = len(self.key)
        top = (1 << (32 + ehb)) - 1
        base = (1 << 32) - n // 2 if ehb else 0                             # (ehb > 0: the entries cross 2^32)
        self.entry = (np.uint64(base) + rng.permutation(n).astype(np.uint64))
        if ehb > 1:                                                         # ... and every other one has its top bit set
            self.entry[::2] += np.uint64((1 << (32 + ehb)) - (1 << 33))
        assert n <= top + 1 and int(self.entry.max()) <= top
        self.carried = rng.integers(0, 1 << carry, size=n).astype(np.uint8) if carry else np.zeros(n, dtype=np.uint8)

    def args(self):
        return self.bucket_begin, self.key, self.entry, self.carried

    def cell_sizes(self):
        c = cells(self.bucket_begin, self.key)
        return (c[:, 1] - c[:, 0]).astype(np.int64)


def _low(rng, n, distinct=None, odd=None):
    """n low keys with ties (about three records per value unless `distinct` says how many values)"""
    d = max(1, n // 3) if distinct is None else distinct
    pool = rng.integers(0, 1 << 32, size=d, dtype=np.uint64)
    if odd is not None:
        pool = (pool & ~np.uint64(1)) | np.uint64(odd)
    return pool[rng.integers(0, d, size=n)]


def cases():
    rng = np.random.default_rng(7)
    out = {}

    def add(name, buckets, check, **kw):
        c = Case(name, buckets, seed=len(out), **kw)
        assert check(c), f"case {name} does not reach the edge it is named for"
        out[name] = c

    sizes = [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    add("cell_sizes_at_the_tile", [[(10 + i, _low(rng, s)) for i, s in enumerate(sizes)]], lambda c: list(c.cell_sizes()) == sizes)
    add("one_top_byte_in_a_bucket", [[(3, _low(rng, 500)), (9, _low(rng, 300))], [(0x42, _low(rng, 20001))], [(1, _low(rng, 77))]],
        lambda c: list(c.cell_sizes()) == [500, 300, 20001, 77])
    add("all_256_top_bytes_once", [[(t, _low(rng, 1)) for t in range(256)], [(5, _low(rng, 9))]],
        lambda c: list(c.cell_sizes()) == [1] * 256 + [9])
    ones = np.full(1000, 0xFFFFFFFF, dtype=np.uint64)
    add("top_00_and_ff_all_ones_low_keys",
        [[(0x00, np.concatenate([_low(rng, 700), np.zeros(50, dtype=np.uint64)])), (0xFF, np.concatenate([ones, _low(rng, 333)]))],
         [(0xFF, np.concatenate([ones[:TILE // 2], _low(rng, TILE + 5)]))]],
        lambda c: set(np.unique(c.key >> np.uint64(32))) == {0, 0xFF} and int((c.key == np.uint64((0xFF << 32) | 0xFFFFFFFF)).sum()) > 1000
        and all(s % TILE for s in c.cell_sizes()))
    add("empty_bucket_between_two", [[(7, _low(rng, 100)), (8, _low(rng, 5))], [], [(7, _low(rng, 60))]],
        lambda c: c.bucket_begin[1] == c.bucket_begin[2] and len(c.bucket_begin) == 4)
    add("one_bucket", [[(0x20, _low(rng, 40)), (0x21, _low(rng, 3))]], lambda c: len(c.bucket_begin) == 2)
    res = [1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 13]
    add("cell_begins_of_every_residue_mod_4", [[(30 + i, _low(rng, s)) for i, s in enumerate(res)], [(1, _low(rng, 6)), (2, _low(rng, 7))]],
        lambda c: {int(b) % 4 for b in cells(c.bucket_begin, c.key)[:, 0]} == {0, 1, 2, 3}
        and {int(e) % 4 for e in cells(c.bucket_begin, c.key)[:, 1]} == {0, 1, 2, 3})

    def tie_crosses_tile(c):   # a group of equal keys with members on both sides of a tile end inside its cell
        e, f = referee_numpy(*c.args())
        for b, en, _ in cells(c.bucket_begin, c.key):
            for t in range(int(b) + TILE, int(en), TILE):
                if not f[t] & 1:
                    return True
        return False
    add("tied_group_across_a_tile_end", [[(4, _low(rng, 40000, distinct=5, odd=1)), (5, _low(rng, 100))], [(4, _low(rng, 2 * TILE, distinct=2, odd=0))]],
        tie_crosses_tile)
    L = np.uint64(0x80000001)   # (odd: the key continues behind its bits, so the groups are open)
    below = rng.integers(0, 0x80000000, size=300, dtype=np.uint64)
    above = rng.integers(0x80000002, 1 << 32, size=300, dtype=np.uint64)

    def tie_at_cell_border(c):  # equal low 32 bits on the last slot of one cell and the first of the next: two groups
        e, f = referee_numpy(*c.args())
        k = np.sort(c.key[:int(c.bucket_begin[1])])
        cs = cells(c.bucket_begin, c.key)
        edge = int(cs[0][1])
        return (k[edge - 1] & np.uint64(0xFFFFFFFF)) == L == (k[edge] & np.uint64(0xFFFFFFFF)) and k[edge - 2] == k[edge - 1] and k[edge] == k[edge + 1] \
            and f[edge] & 1 and not f[edge - 1] & 1 and not f[edge + 1] & 1
    add("tied_groups_meet_at_a_cell_border", [[(5, np.concatenate([below, np.full(3, L)])), (6, np.concatenate([np.full(4, L), above]))]],
        tie_at_cell_border)
    for ehb, carry in ((1, 5), (3, 5), (8, 0), (1, 0), (2, 6), (3, 0), (0, 6)):
        add(f"entry_high_bits_{ehb}_carried_{carry}", [[(t, _low(rng, 700)) for t in (0, 9, 0xFE)], [(0xFF, _low(rng, TILE + 77))]],
            (lambda c: ehb == 0 or (int(c.entry.min()) < (1 << 32) <= int(c.entry[1::2].max()) and int(c.entry.max()) >> (31 + ehb) == 1
                                    and len(np.unique(c.entry)) == len(c.entry))),
            ehb=ehb, carry=carry)
    add("cell_table_of_258_cells", [[(t, _low(rng, 1 + t % 5)) for t in range(256)], [(1, _low(rng, 2)), (200, _low(rng, 2))]],
        lambda c: len(cells(c.bucket_begin, c.key)) == 258)
    return out
