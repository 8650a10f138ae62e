"""A CPU referee for the device-wide scan (scan.h) and the stable tile ranks (stable_tiles.h), and the inputs that drive them to
their edges.

Plain Python and numpy in exact integers, written from the contract in the comments of scan.h, stable_tiles.h and of the operators
themselves; it shares no code with the library.  Test infrastructure (a helper module, not a conftest).

The contract:

  scan     exclusive[i] = fold(items[:i]), inclusive[i] = fold(items[:i + 1]), total = fold(items), where fold starts from the
           kind's identity and combines from the left.  `fold` below IS that definition, item by item; `scan` computes the same
           arrays with numpy (a million DocMax items take the definition minutes).  tests/test_scan_referee.py holds the two together.
  kinds    the value / operator pairs production instantiates (the numbers are CDB_DEBUG_SCAN_* of include/coffeedb_gpu.h):
           U64_ADD   a + b modulo 2^64                                            identity 0
           U64_MAX   max(a, b)                                                    identity 0
           U2_ADD    (a.a + b.a, a.b + b.b), each modulo 2^64                     identity (0, 0)
           U2_SUMMAX (a.a + b.a modulo 2^64, max(a.b, b.b))                       identity (0, 0)
           DOCMAX    "segmented max": (b.doc, max(a.mx, b.mx) if a.doc == b.doc else b.mx)
                     identity (2^64 - 1, 0) — a LEFT identity only: combined from the right it wipes the maximum
           FLAGS_ADD U2_ADD over flag bytes f decoded as u = f >> 1 & 1, item = (u, u & f & 1)
  DOCMAX   is associative — and a device scan, which regroups the fold, equal to it — only where equal documents are adjacent (the
           hit list it scans is sorted by document).  Every DOCMAX input built here keeps them adjacent.  Its total is not part of
           the contract: the device pads the last tile with the identity on the right, and production discards what comes back.
  ranks    before[i] = flagged slots in front of slot i (an exclusive cumsum of the flags), tile_base[t] = before[t * 4096],
           total = flagged slots.

The geometry constants are data about the kernels under test, copied by hand from scan.h and stable_tiles.h — not an import.
"""
import zlib

import numpy as np

M64 = (1 << 64) - 1
U64_ADD, U64_MAX, U2_ADD, U2_SUMMAX, DOCMAX, FLAGS_ADD = range(6)
KINDS = (U64_ADD, U64_MAX, U2_ADD, U2_SUMMAX, DOCMAX, FLAGS_ADD)
KIND_NAMES = ("u64_add", "u64_max", "u2_add", "u2_summax", "docmax", "flags_add")
PAIR_KINDS = (U2_ADD, U2_SUMMAX, DOCMAX, FLAGS_ADD)
IDENTITY = {U64_ADD: 0, U64_MAX: 0, U2_ADD: (0, 0), U2_SUMMAX: (0, 0), DOCMAX: (M64, 0), FLAGS_ADD: (0, 0)}

IPT, WAVE, TILE = 16, 64 * 16, 256 * 16      # items per thread, per wave, per tile of the scan (SC_IPT, 64 SC_IPT, SC_TILE)
SWEEP = 1024 * 16                            # partials one sweep of scan_partials_kernel covers (SP_NT * SC_IPT)
LEVEL = 1 << 16                              # partials beyond which scan_partials_inplace scans them like data
ST_ROUNDS, ST_TILE = 16, 4096                # stable_tiles.h: rounds per tile, slots per tile (256 threads x 16 rounds)

SCAN_SIZES = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096, 3 * 4096 + 1, 257 * 4096 + 1)
PARTIALS_SIZES = (0, 1, SWEEP - 1, SWEEP, SWEEP + 1, 2 * SWEEP + 1, LEVEL - 1, LEVEL, LEVEL + 1, 17 * 4096 - 1, 17 * 4096, 17 * 4096 + 1)
PARTIALS_KINDS = (U64_ADD, U2_ADD, U64_MAX, DOCMAX)
RANK_SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1)
RANK_BIG = 4097 * 4096 + 3                   # the tile counts themselves cross a scan tile


def combine(kind, a, b):
    """the operator, on Python ints / pairs of them"""
    if kind == U64_ADD:
        return (a + b) & M64
    if kind == U64_MAX:
        return a if a > b else b
    if kind in (U2_ADD, FLAGS_ADD):
        return ((a[0] + b[0]) & M64, (a[1] + b[1]) & M64)
    if kind == U2_SUMMAX:
        return ((a[0] + b[0]) & M64, a[1] if a[1] > b[1] else b[1])
    if kind == DOCMAX:
        return (b[0], (a[1] if a[1] > b[1] else b[1]) if a[0] == b[0] else b[1])
    raise ValueError(kind)


def decode_flags(flags):
    """flag bytes -> the (n, 2) items FLAGS_ADD sums"""
    f = np.asarray(flags, dtype=np.uint8).astype(np.uint64)
    u = (f >> np.uint64(1)) & np.uint64(1)
    return np.stack([u, u & f & np.uint64(1)], axis=1) if len(f) else np.zeros((0, 2), dtype=np.uint64)


def _items(kind, items):
    if kind == FLAGS_ADD:
        return decode_flags(items)
    a = np.asarray(items, dtype=np.uint64)
    return a.reshape((-1, 2)) if kind in PAIR_KINDS else a.reshape(-1)


def _to_py(kind, x):
    return (int(x[0]), int(x[1])) if kind in PAIR_KINDS else int(x)


def _total_array(kind, t):
    return np.array(t, dtype=np.uint64)


def fold(kind, items):
    """(exclusive, inclusive, total) by the definition: one left fold in Python integers"""
    a = _items(kind, items)
    ex, inc = np.zeros_like(a), np.zeros_like(a)
    acc = IDENTITY[kind]
    for i in range(len(a)):
        ex[i] = acc
        acc = combine(kind, acc, _to_py(kind, a[i]))
        inc[i] = acc
    return ex, inc, _total_array(kind, acc)


def _docmax_inclusive(a):
    """running maximum inside runs of equal adjacent documents, exactly: the maxima are replaced by their ranks among the distinct
    values (an order-preserving map into [0, n)), so that run number * n + rank fits an int64 and ONE running maximum over that
    key restarts by itself wherever a new run begins"""
    n = len(a)
    doc, mx = a[:, 0], a[:, 1]
    values, rank = np.unique(mx, return_inverse=True)
    run = np.zeros(n, dtype=np.int64)
    run[1:] = np.cumsum(doc[1:] != doc[:-1])
    key = np.maximum.accumulate(run * n + rank.astype(np.int64))
    return np.stack([doc, values[key - run * n]], axis=1)


def scan(kind, items):
    """(exclusive, inclusive, total) like fold(), computed with numpy (uint64 arithmetic wraps modulo 2^64 by itself)"""
    a = _items(kind, items)
    n = len(a)
    if n == 0:
        return a.copy(), a.copy(), _total_array(kind, IDENTITY[kind])
    with np.errstate(over="ignore"):
        if kind == U64_ADD:
            inc = np.cumsum(a, dtype=np.uint64)
        elif kind == U64_MAX:
            inc = np.maximum.accumulate(a)
        elif kind in (U2_ADD, FLAGS_ADD):
            inc = np.cumsum(a, axis=0, dtype=np.uint64)
        elif kind == U2_SUMMAX:
            inc = np.stack([np.cumsum(a[:, 0], dtype=np.uint64), np.maximum.accumulate(a[:, 1])], axis=1)
        elif kind == DOCMAX:
            inc = _docmax_inclusive(a)
        else:
            raise ValueError(kind)
    ex = np.empty_like(inc)
    ex[0] = IDENTITY[kind]
    ex[1:] = inc[:-1]
    return ex, inc, inc[-1].copy()


def stable_ranks(flags):
    """(before[n], tile_base[ceil(n / 4096)], total) of flag bytes (non-zero = flagged)"""
    f = (np.asarray(flags, dtype=np.uint8) != 0).astype(np.uint64)
    inc = np.cumsum(f, dtype=np.uint64)
    before = inc - f
    return before, before[::ST_TILE].copy(), int(inc[-1]) if len(f) else 0


# ------------------------------------------------------------------------------------------------------------------------
# scan inputs.  Every builder returns {name: items}; sizes too small for a pattern simply leave it out.
# ------------------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([zlib.crc32(x.encode()) if isinstance(x, str) else int(x) for x in seed])


def boundary_positions(n):
    """item positions at every thread, wave and tile boundary of the scan, and one item either side"""
    pos = set()
    for unit in (IPT, WAVE, TILE):
        for b in range(unit, n + 1, unit):
            pos.update((b - 1, b, b + 1))
    return np.array(sorted(p for p in pos if 0 < p < n), dtype=np.int64)


def _docs_from_starts(n, starts, first=0):
    """ascending document ids: a new document begins at every position in `starts`"""
    head = np.zeros(n, dtype=np.uint64)
    head[np.asarray(starts, dtype=np.int64)] = 1
    return np.cumsum(head, dtype=np.uint64) + np.uint64(first)


def u64_inputs(kind, n):
    r = _rng("u64", kind, n)
    out = {"identity": np.zeros(n, dtype=np.uint64), "ones": np.ones(n, dtype=np.uint64),
           "small": r.integers(0, 1000, n, dtype=np.uint64)}
    if kind == U64_ADD:
        out["wrap"] = (np.uint64(1) << np.uint64(63)) - np.uint64(3) + r.integers(0, 7, n, dtype=np.uint64)
    else:
        base = r.integers(1, 1000, n, dtype=np.uint64)
        big = np.uint64(M64)
        for name, at in (("max_first", 0), ("max_last", n - 1), ("max_lane63", min(n - 1, WAVE - 1)), ("max_tile_end", min(n - 1, TILE - 1)),
                         ("max_second_tile_end", 2 * TILE - 1), ("max_wave2", 2 * WAVE + 5)):
            if 0 <= at < n:
                a = base.copy()
                a[at] = big
                out[name] = a
        out["rising"] = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)   # every item is a new maximum
    return out


def u2_inputs(kind, n):
    r = _rng("u2", kind, n)
    out = {"identity": np.zeros((n, 2), dtype=np.uint64), "ones": np.ones((n, 2), dtype=np.uint64),
           "small": r.integers(0, 1000, (n, 2), dtype=np.uint64)}
    wrap = (np.uint64(1) << np.uint64(63)) - np.uint64(3) + r.integers(0, 7, (n, 2), dtype=np.uint64)
    if kind == U2_SUMMAX:
        wrap[:, 1] = r.integers(0, 1 << 62, n, dtype=np.uint64)
        # the maximum lies in another tile (wave, thread) than the items that must still see it
        for name, at in (("max_first", 0), ("max_first_tile", TILE // 2), ("max_wave2", 2 * WAVE + 5), ("max_last", n - 1)):
            if 0 <= at < n:
                a = r.integers(0, 1000, (n, 2), dtype=np.uint64)
                a[at, 1] = np.uint64(M64)
                out[name] = a
    out["wrap"] = wrap
    return out


def docmax_inputs(n):
    """documents stay adjacent in every input (see the module text); only `identity` uses the identity's document id 2^64 - 1"""
    r = _rng("docmax", n)
    mx = r.integers(0, 1 << 40, n, dtype=np.uint64)
    ar = np.arange(n, dtype=np.uint64)
    out = {"identity": np.stack([np.full(n, M64, dtype=np.uint64), np.zeros(n, dtype=np.uint64)], axis=1),
           "zeros": np.zeros((n, 2), dtype=np.uint64),                                                        # document 0, maximum 0
           "ones": np.ones((n, 2), dtype=np.uint64),
           "one_document": np.stack([np.full(n, 7, dtype=np.uint64), mx], axis=1),
           "every_item_new": np.stack([ar * np.uint64(3) + np.uint64(1), mx], axis=1),
           "small_runs": np.stack([_docs_from_starts(n, np.flatnonzero(r.random(n) < 0.2)), r.integers(0, 50, n, dtype=np.uint64)], axis=1),
           # one document whose maximum falls from item to item: every later item must keep the first one's
           "decreasing": np.stack([np.full(n, 5, dtype=np.uint64), np.uint64(1 << 41) - ar], axis=1)}
    b = boundary_positions(n)
    for off, name in ((-1, "starts_before_boundary"), (0, "starts_at_boundary"), (1, "starts_after_boundary")):
        s = b[(b - off) % IPT == 0]      # (wave and tile boundaries are thread boundaries too)
        if len(s):
            out[name] = np.stack([_docs_from_starts(n, s), mx], axis=1)     # document ids from 0: the first one IS document 0
    if n > TILE + 1:
        # a long document whose largest maximum lies in an earlier tile than its last item, in front of and behind short ones
        a = np.stack([_docs_from_starts(n, [3, n - 2]), r.integers(0, 1000, n, dtype=np.uint64)], axis=1)
        a[5, 1] = np.uint64(1 << 50)
        out["max_in_earlier_tile"] = a
    return out


def flag_inputs(n):
    """bytes 0..3; `across_loads` puts every ordered pair of them on the last byte of one 16-byte load and the first of the next"""
    r = _rng("flags", n)
    out = {"identity": np.zeros(n, dtype=np.uint8), "ones": np.ones(n, dtype=np.uint8), "threes": np.full(n, 3, dtype=np.uint8),
           "random": r.integers(0, 4, n, dtype=np.uint8)}
    a = r.integers(0, 4, n, dtype=np.uint8)
    edge = np.arange(16, n, 16, dtype=np.int64)        # first byte of every load but the first
    k = np.arange(len(edge))
    a[edge - 1] = k % 4
    a[edge] = (k // 4) % 4
    out["across_loads"] = a
    return out


def scan_inputs(kind, n):
    if kind in (U64_ADD, U64_MAX):
        return u64_inputs(kind, n)
    if kind in (U2_ADD, U2_SUMMAX):
        return u2_inputs(kind, n)
    return docmax_inputs(n) if kind == DOCMAX else flag_inputs(n)


def partials_inputs(kind, nb):
    """raw tile sums for scan_partials_inplace: {name: sums}"""
    r = _rng("partials", kind, nb)
    if kind == U64_ADD:
        return {"ones": np.ones(nb, dtype=np.uint64), "random": r.integers(0, 1 << 63, nb, dtype=np.uint64)}
    if kind == U2_ADD:
        return {"ones": np.ones((nb, 2), dtype=np.uint64), "random": r.integers(0, 1 << 63, (nb, 2), dtype=np.uint64)}
    if kind == U64_MAX:
        return {"rising": np.arange(nb, dtype=np.uint64) + np.uint64(1), "random": r.integers(0, 1 << 63, nb, dtype=np.uint64)}
    mx = r.integers(0, 1 << 40, nb, dtype=np.uint64)
    return {"one_document": np.stack([np.full(nb, 9, dtype=np.uint64), mx], axis=1),
            "runs": np.stack([_docs_from_starts(nb, np.flatnonzero(r.random(nb) < 0.01)), mx], axis=1)}


# ------------------------------------------------------------------------------------------------------------------------
# flag layouts of the stable ranks: slot i of tile t is handled by thread (i % 256) — wave (i % 256) // 64, lane i % 64 — in
# round (i % 4096) // 256
# ------------------------------------------------------------------------------------------------------------------------
SINGLE_SLOTS = (0, 63, 64, 255, 256, 4095, 4096)


def rank_patterns(n):
    r = _rng("ranks", n)
    i = np.arange(n, dtype=np.int64)
    lane, wave, rnd = i % 64, (i % 256) // 64, (i % ST_TILE) // 256
    out = {"none": np.zeros(n, dtype=np.uint8), "all": np.ones(n, dtype=np.uint8), "alternating": (i & 1).astype(np.uint8),
           "lane0": (lane == 0).astype(np.uint8), "lane63": (lane == 63).astype(np.uint8), "wave3": (wave == 3).astype(np.uint8),
           "round0": (rnd == 0).astype(np.uint8), "round15": (rnd == 15).astype(np.uint8), "odd_rounds": (rnd & 1).astype(np.uint8)}
    for at in sorted(set(SINGLE_SLOTS) | {n - 1}):
        if 0 <= at < n:
            f = np.zeros(n, dtype=np.uint8)
            f[at] = 1
            out[f"single_{at}"] = f
    for pct in (1, 50, 99):
        out[f"random_{pct}"] = (r.random(n) < pct / 100.0).astype(np.uint8) * np.uint8(1 + pct % 3)   # (any non-zero byte is a flag)
    return out
