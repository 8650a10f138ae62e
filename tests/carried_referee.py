"""CPU referee of the in-place carried round (coffeedb_amd/csrc/carried_inplace.h: sa_carried_inplace_kernel), and the cases
its tests run.  The rule is stated twice, once in Python integers (inplace_ints) and once in numpy (inplace_numpy);
tests/test_carried_referee.py holds the two equal, tests/test_gpu_carried_inplace.py holds the kernel equal to them.

The rule.  Slot i has an entry and a flag byte: bit 0 = head of a group, bit 1 = open, bits 2.. = the entry's carried bits,
of which the low x are the sort key.  The array is cut into tiles of TILE slots.  Inside a tile the OPEN slots, in order,
form groups: an open head and the open non-heads behind it up to the next open head.  A group is OWNED by its tile when
    * it has a head in the tile (open non-heads in front of the tile's first open head belong to the previous tile's group),
    * it ends in the tile: it is not the tile's last group, or the tile's last slot is not its last member, or the array ends
      behind the tile, or the slot behind the tile is not an open non-head,
    * it has at most GROUP_MAX members.
An owned group's entries are sorted stably by their key; the carried bits (all of bits 2..) travel with the entry.  The flag of
a slot of an owned group becomes head' | open' << 1 | carried << 2 with head' = old head of the slot or key differs from the
sorted predecessor's, last' = last slot of the group or head' of the next slot, open' = not (head' and last').  Everything
else stays as it was.  Beside the arrays: per tile (open entries, open heads) as left, the number of open entries met, and
the number of slots whose occupant changed."""
import numpy as np

TILE = 4096
GROUP_MAX = 64
TILES_PER_WAVE = 4          # FC_TILES_PER_WAVE
TILES_PER_WORKGROUP = 16    # four waves
LIST_WINDOW = 1024          # CI_LIST


def inplace_ints(entries, flags, x, tile=TILE, group_max=GROUP_MAX):
    """-> (entries, flags, partials [(open, heads)], met, moved, info); info counts what the rule met"""
    e0, f0 = [int(v) for v in entries], [int(v) for v in flags]
    n = len(e0)
    e, f = list(e0), list(f0)
    mask = (1 << x) - 1
    partials, met, moved = [], 0, 0
    info = dict(owned=0, long=0, crossing=0, headless=0, settled=0, kept_open=0, sizes=set())
    for t0 in range(0, n, tile):
        t1 = min(t0 + tile, n)
        groups, cur = [], None
        for i in range(t0, t1):
            if not f0[i] & 2:
                continue
            met += 1
            if f0[i] & 1:
                cur = [i]
                groups.append(cur)
            elif cur is not None:
                cur.append(i)
            else:
                info["headless"] += 1
        for gi, g in enumerate(groups):
            if len(g) > group_max:
                info["long"] += 1
                continue
            if gi == len(groups) - 1 and g[-1] == t0 + tile - 1 and g[-1] + 1 < n and f0[g[-1] + 1] & 3 == 2:
                info["crossing"] += 1
                continue
            info["owned"] += 1
            info["sizes"].add(len(g))
            keys = [(f0[i] >> 2) & mask for i in g]
            order = sorted(range(len(g)), key=lambda j: keys[j])  # (sorted is stable)
            heads = []
            for p, j in enumerate(order):
                e[g[p]] = e0[g[j]]
                moved += p != j
                heads.append(bool(f0[g[p]] & 1) or (p > 0 and keys[j] != keys[order[p - 1]]))
            for p, j in enumerate(order):
                last = p == len(g) - 1 or heads[p + 1]
                opn = not (heads[p] and last)
                f[g[p]] = int(heads[p]) | (int(opn) << 1) | ((f0[g[j]] >> 2) << 2)
                info["settled" if not opn else "kept_open"] += 1
        partials.append((sum(1 for i in range(t0, t1) if f[i] & 2), sum(1 for i in range(t0, t1) if f[i] & 3 == 3)))
    return e, f, partials, met, moved, info


def inplace_numpy(entries, flags, x, tile=TILE, group_max=GROUP_MAX):
    """the same rule on whole arrays -> (entries, flags, partials uint64[tiles, 2], met, moved)"""
    e0 = np.asarray(entries, dtype=np.uint64)
    f0 = np.asarray(flags, dtype=np.uint8)
    n = len(e0)
    ntiles = (n + tile - 1) // tile
    e, f = e0.copy(), f0.copy()
    P = np.flatnonzero(f0 & 2)                      # open slots, in order
    met = len(P)
    moved = 0
    if met:
        head = (f0[P] & 1).astype(np.int64)
        tl = P // tile
        # heads so far in the slot's own tile (0: head-less leading member)
        cum = np.cumsum(head)
        first_of_tile = np.flatnonzero(np.r_[True, tl[1:] != tl[:-1]])
        before_tile = np.repeat((cum - head)[first_of_tile], np.diff(np.r_[first_of_tile, met]))
        c = cum - before_tile
        gid = tl * (tile + 1) + c                   # ascends with the slot
        _, inv, counts = np.unique(gid, return_inverse=True, return_counts=True)
        size = counts[inv]
        own = (c > 0) & (size <= group_max)
        # the last group of a tile that goes on behind the tile's last slot
        last_of_tile = np.r_[first_of_tile[1:] - 1, met - 1]
        lp = P[last_of_tile]
        nxt = np.minimum(lp + 1, n - 1)
        cross = (lp % tile == tile - 1) & (lp + 1 < n) & ((f0[nxt] & 3) == 2)
        own &= ~np.isin(gid, gid[last_of_tile[cross]])
        Q = P[own]                                  # the owned slots = the destinations, group by group
        if len(Q):
            g = gid[own]
            key = ((f0[Q] >> 2) & ((1 << x) - 1)).astype(np.int64)
            order = np.lexsort((np.arange(len(Q)), key, g))   # stable inside every group
            S = Q[order]                            # S[k] -> Q[k]
            skey = key[order]
            same_prev = np.r_[False, g[1:] == g[:-1]]
            nhead = ((f0[Q] & 1) != 0) | (same_prev & np.r_[False, skey[1:] != skey[:-1]])
            last = np.r_[~same_prev[1:] | nhead[1:], True]
            nopen = ~(nhead & last)
            e[Q] = e0[S]
            f[Q] = nhead.astype(np.uint8) | (nopen.astype(np.uint8) << 1) | ((f0[S] >> 2) << 2)
            moved = int(np.count_nonzero(e[Q] != e0[Q]))
    partials = np.zeros((ntiles, 2), dtype=np.uint64)
    idx = np.arange(n) // tile
    partials[:, 0] = np.bincount(idx[(f & 2) != 0], minlength=ntiles)
    partials[:, 1] = np.bincount(idx[(f & 3) == 3], minlength=ntiles)
    return e, f, partials, met, moved


def carried_round(entries, flags, x):
    """the whole carried round as the list machinery runs it: every open group of the ARRAY (no tiles, no size limit) sorted
    stably by its key; the flag of every open slot rewritten as head' | open' << 1 (sa_place, CARRIED) -> (entries, flags)"""
    e0, f0 = [int(v) for v in entries], [int(v) for v in flags]
    e, f = list(e0), list(f0)
    mask = (1 << x) - 1
    P = [i for i in range(len(e0)) if f0[i] & 2]
    groups = []
    for i in P:
        if f0[i] & 1 or not groups:
            groups.append([i])
        else:
            groups[-1].append(i)
    for g in groups:
        keys = [(f0[i] >> 2) & mask for i in g]
        order = sorted(range(len(g)), key=lambda j: keys[j])
        heads = [bool(f0[g[p]] & 1) or (p > 0 and keys[j] != keys[order[p - 1]]) for p, j in enumerate(order)]
        for p, j in enumerate(order):
            e[g[p]] = e0[g[j]]
            last = p == len(g) - 1 or heads[p + 1]
            f[g[p]] = int(heads[p]) | (int(not (heads[p] and last)) << 1)
    return e, f


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def _entries(n, rng):
    """distinct 40-bit entries with non-zero high bytes"""
    lo = rng.permutation(n).astype(np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)
    hi = (rng.integers(1, 256, size=n)).astype(np.uint64)
    return (hi << np.uint64(32)) | lo


class Layout:
    """an array of closed singletons (head bit, random live carried bits) into which groups are put"""

    def __init__(self, n, x, seed):
        self.n, self.x = n, x
        self.rng = np.random.default_rng(seed)
        self.entries = _entries(n, self.rng)
        self.flags = (1 | (self.rng.integers(0, 64, size=n) << 2)).astype(np.uint8)

    def group(self, start, keys, open_=True, high=0):
        """a group at slots [start, start + len(keys)): head first; `high` = bits above the key that must travel too"""
        keys = np.asarray(keys, dtype=np.int64)
        m = len(keys)
        assert 0 <= start and start + m <= self.n and np.all(keys < (1 << self.x))
        carried = (keys | (high << self.x)) & 63
        fl = (carried << 2) | (2 if open_ else 0)
        fl[0] |= 1
        self.flags[start:start + m] = fl.astype(np.uint8)
        return self

    def headless(self, start, keys):
        """open non-heads without a head in front (what a tile sees of the previous tile's group)"""
        keys = np.asarray(keys, dtype=np.int64)
        self.flags[start:start + len(keys)] = ((keys << 2) | 2).astype(np.uint8)
        return self

    def done(self):
        return self.entries, self.flags, self.x


def _keys(kind, m, x, rng):
    top = 1 << x
    if kind == "equal":
        return np.full(m, top - 1)
    if kind == "distinct":          # needs m <= 2^x
        return rng.permutation(top)[:m]
    if kind == "descending":        # strictly, as far as the key space allows; then wrapped runs of descents
        return (top - 1 - np.arange(m)) % top if m <= top else np.sort(rng.integers(0, top, size=m))[::-1]
    if kind == "two":               # two values interleaved, the greater first: stability on both
        return np.where(np.arange(m) % 2 == 0, top - 1, 0)
    return rng.integers(0, top, size=m)


def cases():
    """name -> (entries, flags, x); every name says which edge the case is there for (tests/test_carried_referee.py checks it)"""
    out = {}
    rng = np.random.default_rng(2024)
    # array lengths, every slot in small random groups
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 1,
              (TILES_PER_WAVE + 1) * TILE - 5, (TILES_PER_WORKGROUP + 1) * TILE - 7):
        L = Layout(n, 3, n)
        i = k = 0
        while i < n:
            m = min(n - i, (2, 3, 4, 1)[k % 4])
            L.group(i, _keys("random", m, 3, rng), open_=m > 1 or n == 1, high=int(rng.integers(0, 8)))
            i += m
            k += 1
        out[f"len_{n}"] = L.done()
    # group sizes x key patterns
    for m in (2, 3, 63, 64, 65):
        for kind in ("equal", "distinct", "descending", "two", "random"):
            x = 6 if kind in ("distinct", "descending") else 3
            if kind == "distinct" and m > 64:
                continue
            L = Layout(3 * TILE + 99, x, m * 7 + len(kind))
            for start in (5, TILE + 100, 2 * TILE + 7, 3 * TILE + 99 - m):   # (the last one ends on the array's last slot)
                L.group(start, _keys(kind, m, x, rng))
            out[f"size_{m}_{kind}"] = L.done()
    # carried widths
    for x in range(1, 7):
        L = Layout(2 * TILE + 3, x, 100 + x)
        i = 3
        while i + 8 < L.n:
            m = int(rng.integers(2, 8))
            L.group(i, _keys("random", m, x, rng), high=int(rng.integers(0, 1 << (6 - x))))
            i += m + int(rng.integers(0, 5))
        out[f"x_{x}"] = L.done()
    # placement against the tile
    L = Layout(3 * TILE, 3, 7)
    L.group(TILE - 1, [5, 1, 3])                       # head on a tile's last slot: runs into the next tile
    L.group(2 * TILE - 3, [4, 2, 0]).group(2 * TILE, [3, 1])  # ends on a tile's last slot, a head first in the next tile
    out["head_on_tile_last_slot"] = L.done()
    L = Layout(3 * TILE, 3, 8)
    L.group(2 * TILE - 3, [4, 2, 0])                   # ends on a tile's last slot, a closed singleton behind
    L.group(3 * TILE - 2, [6, 1])                      # ends on the array's last slot
    out["ends_on_tile_last_slot"] = L.done()
    L = Layout(4 * TILE + 9, 4, 9)
    L.group(TILE - 10, _keys("random", TILE + 30, 4, rng))     # spans more than a whole tile
    L.group(2 * TILE + 40, [3, 1, 2])                  # (an owned group behind its head-less tail)
    out["group_spans_a_tile"] = L.done()
    L = Layout(2 * TILE, 3, 10)
    L.headless(0, [7, 0, 3]).group(3, [2, 1])          # head-less at the array's start and at a tile's
    L.group(TILE - 2, [7, 7, 6, 5, 4, 3]).group(TILE + 4, [1, 0])
    out["headless_leading_members"] = L.done()
    # the 64-entry trips of the list: a group across list position 64 at every offset, small groups in front of it
    for o in range(1, 64):
        m = min(64, o + 2)
        L = Layout(TILE + 300, 5, 500 + o)
        lead = 64 - o
        i, left = 2, lead
        while left:
            k = 3 if left % 2 == 1 and left >= 3 else min(left, 2)   # (a lone entry in front: an open group of one)
            L.group(i, _keys("descending", k, 5, rng))
            i += k + 1
            left -= k
        L.group(i, _keys("random", m, 5, rng))
        L.group(i + m + 2, [9, 4, 4, 1])               # (and the trip behind it)
        out[f"trip_boundary_{o}"] = L.done()
    # long groups in front of and behind short ones, in one tile (the long ones are passed over 64 entries at a time)
    L = Layout(TILE, 5, 11)
    L.group(1, [3, 1]).group(10, _keys("random", 65, 5, rng)).group(75, [9, 2, 5])
    L.group(200, _keys("random", 64, 5, rng)).group(264, _keys("random", 200, 5, rng)).group(464, [8, 7])
    out["long_between_short"] = L.done()
    # what must come back untouched
    L = Layout(2 * TILE + 50, 3, 12)
    for start in range(4, 2 * TILE, 37):
        L.group(start, _keys("descending", 5, 3, rng), open_=False)   # closed groups of several, live bits 2..
    out["closed_groups_live_bits"] = L.done()
    L = Layout(3 * TILE, 3, 13)
    L.group(TILE + 5, [4, 0])                          # tiles 0 and 2: nothing open
    out["tiles_with_nothing_open"] = L.done()
    L = Layout(3 * TILE, 2, 14)                        # a list that fills a whole tile: tile 1 open throughout
    i = TILE
    while i < 2 * TILE:
        m = int(min(2 * TILE - i, rng.integers(2, 9)))
        L.group(i, _keys("random", m, 2, rng))
        i += m
    out["list_fills_a_tile"] = L.done()
    # lists around the kernel's list window (LIST_WINDOW entries are listed at a time; a trip also needs the entry behind it):
    # the last trip of a tile's list must not begin in a window that ends in front of the list's end
    for total in (LIST_WINDOW - 1, LIST_WINDOW, LIST_WINDOW + 1, LIST_WINDOW + 26, LIST_WINDOW + 63, LIST_WINDOW + 64,
                  LIST_WINDOW + 65, 2 * LIST_WINDOW + 30, 3 * LIST_WINDOW - 70):
        for first in (2, 3, 40):                       # (the first group shifts where the trips fall)
            L = Layout(2 * TILE + 5, 4, total * 3 + first)
            i, left, m = TILE + 1, total, first
            while left:
                m = min(m, left)
                L.group(i, _keys("random", m, 4, rng))
                i += m + int(rng.integers(0, 2))
                left -= m
                m = int(rng.integers(2, 6))
            out[f"window_{total}_{first}"] = L.done()
    L = Layout(2 * TILE, 6, 15)                        # one group of the whole tile
    L.group(0, _keys("random", TILE, 6, rng))
    out["one_group_fills_a_tile"] = L.done()
    return out


def list_positions(flags, tile_index=0, tile=TILE):
    """slot -> position in its tile's list of open slots"""
    f = np.asarray(flags)[tile_index * tile:(tile_index + 1) * tile]
    P = np.flatnonzero(f & 2)
    return {int(p) + tile_index * tile: k for k, p in enumerate(P)}
