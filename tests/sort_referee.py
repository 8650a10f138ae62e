"""A CPU referee for the radix-sort primitive (radix_sort.h), and the inputs that drive it to its edges.

Plain numpy, written from the contract in the comments of radix_sort(), radix_sort_cfg() and radix_sort_split(); it shares no
code with the library.  Test infrastructure (a helper module, not a conftest).

The contract:

  plain sort   stable by the key field (key >> begin_bit) & mask(end_bit - begin_bit); keys travel with ALL their bits, values
               with their keys.
  split sort   records (u32 key, value, auxiliary word); stable by the composite
               ((key & mask(hi_bits)) << 8 lead) | (aux & mask(8 lead)); the auxiliary bytes above the `lead` sort digits and the
               key bits above hi_bits are carried along untouched.
  passes       digit p of the sort field is its bits [dbits p, dbits (p + 1)) (the last digit may be narrower); a split sort has its
               `lead` auxiliary bytes as digits in front of the key digits.  A pass is skipped exactly when one digit value holds
               all n elements — unless the histograms were counted on the device, where the host never sees them: none is skipped.
  workspace    every executed pass takes the next epoch, 1..255; behind 255 the tags wrap and the next pass is epoch 1 again.

CONFIGS is data about the contract under test (threads per workgroup, keys per thread of every kernel configuration), copied by
hand from the configuration block and the variant table of radix_sort.h (RsBig / RsMid / RsSmall and their ballot twins,
RsKeyBig / RsKeySmall, RS_SPLIT_BIG_IPT; RS_VARIANT_*, rs_dispatch_variant) — not an import from them.
"""
import numpy as np

M64 = (1 << 64) - 1
MAX_PASSES = 16
PRODUCTION_VARIANTS = (1, 26, 21, 32, 36, 33)      # what variant 0 resolves to (31 = 33 + the XCD-aware tile order)
AB_VARIANTS = (4, 41)                              # kept for A/B measurements, 64-bit keys only

# configuration -> (threads per workgroup, keys per thread)
CONFIGS = {
    ("pair", 21): (1024, 16), ("pair", 31): (1024, 16), ("pair", 33): (1024, 16), ("pair", 41): (1024, 16),
    ("pair", 26): (256, 18), ("pair", 36): (256, 18),
    ("pair", 1): (256, 15), ("pair", 32): (256, 15), ("pair", 4): (256, 15),
    ("keyonly", "small"): (256, 16), ("keyonly", "big"): (1024, 16),
    # split records: the big tile holds 12 keys per thread when the values have 8 bytes
    ("split4", 21): (1024, 16), ("split4", 31): (1024, 16), ("split4", 33): (1024, 16),
    ("split8", 21): (1024, 12), ("split8", 31): (1024, 12), ("split8", 33): (1024, 12),
    ("split4", 26): (256, 18), ("split4", 36): (256, 18), ("split8", 26): (256, 18), ("split8", 36): (256, 18),
    ("split4", 1): (256, 15), ("split4", 32): (256, 15), ("split8", 1): (256, 15), ("split8", 32): (256, 15),
}
KEYONLY_BIG_N = 1 << 23


def _by_size(n):
    """what variant 0 means for n elements (one-atomic ranking; 31 becomes 33 where the caller may not use the grouped order)"""
    return 31 if n >= (1 << 23) else (36 if n >= (1 << 19) else 32)


def tile_chunk(kind, variant=0, n=0, val_bytes=4):
    """(tile T, wave chunk C = 64 x keys per thread) of a sort of `kind` in "pair", "keyonly", "split" """
    if kind == "keyonly":
        nt, ipt = CONFIGS[("keyonly", "big" if n >= KEYONLY_BIG_N else "small")]
    else:
        if variant == 0:
            variant = _by_size(n)
        nt, ipt = CONFIGS[("pair" if kind == "pair" else f"split{val_bytes}", variant)]
    return nt * ipt, 64 * ipt


def edge_sizes(T, C):
    """the smallest sizes at which a tile of T keys in wave chunks of C can go wrong"""
    return [1, 2, 63, 64, 65, C - 1, C, C + 1, T - C + 1, T - 1, T, T + 1, 2 * T, 3 * T + C + 1]


def tiles(n, T):
    return -(-n // T)


def _mask(bits):
    return (1 << bits) - 1


def _udtype(nbytes):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[nbytes]


# ------------------------------------------------------------------------------------------------------------------------
# the sorts
# ------------------------------------------------------------------------------------------------------------------------
def sort_field(keys, begin, end):
    k = keys.astype(np.uint64)
    return (k >> np.uint64(begin)) & np.uint64(_mask(end - begin))


def plain_perm(keys, begin, end):
    return np.argsort(sort_field(keys, begin, end), kind="stable")


def plain_sort(keys, vals, begin, end):
    """(keys, vals) after the sort; vals may be None"""
    perm = plain_perm(keys, begin, end)
    return keys[perm], (None if vals is None else vals[perm])


def split_field(k32, aux, hi_bits, lead):
    hi = k32.astype(np.uint64) & np.uint64(_mask(hi_bits))
    lo = aux.astype(np.uint64) & np.uint64(_mask(8 * lead))
    return (hi << np.uint64(8 * lead)) | lo


def split_sort(k32, vals, aux, hi_bits, lead):
    perm = np.argsort(split_field(k32, aux, hi_bits, lead), kind="stable")
    return k32[perm], vals[perm], aux[perm]


def _digits(field, nbits, dbits):
    """the digit columns of a sort field of nbits bits, lowest first"""
    out = []
    for p in range(-(-nbits // dbits)):
        w = min(dbits, nbits - dbits * p)
        out.append((field >> np.uint64(dbits * p)) & np.uint64(_mask(w)))
    return out


def _count_passes(cols, device_hist):
    if device_hist:
        return len(cols), 0
    skipped = sum(1 for c in cols if bool((c == c[0]).all()))
    return len(cols) - skipped, skipped


def predict_passes(keys, begin, end, dbits=8, device_hist=False):
    """(passes run, passes skipped) of a plain sort"""
    return _count_passes(_digits(sort_field(keys, begin, end), end - begin, dbits), device_hist)


def predict_passes_split(k32, aux, hi_bits, lead, device_hist=False):
    cols = [(aux.astype(np.uint64) >> np.uint64(8 * p)) & np.uint64(255) for p in range(lead)]
    cols += _digits(k32.astype(np.uint64) & np.uint64(_mask(hi_bits)), hi_bits, 8)
    return _count_passes(cols, device_hist)


def pass_count(begin, end, dbits):
    return -(-(end - begin) // dbits)


def epoch_after(epoch, passes):
    """the workspace's epoch after `passes` more executed passes, and whether the tags wrapped on the way (at which pass)"""
    wrapped_at = None
    for p in range(passes):
        if epoch == 255:
            epoch = 0
            wrapped_at = p
        epoch += 1
    return epoch, wrapped_at


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def _rand_bits(rng, n, nbytes):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64).astype(_udtype(nbytes)) if nbytes == 8 else \
        rng.integers(0, 1 << (8 * nbytes), size=n, dtype=np.uint64).astype(_udtype(nbytes))


PATTERNS = ("uniform", "ones", "ones_sparse", "one_bit", "ascending", "descending", "last_tile_ones")


def pattern_keys(pattern, n, key_bytes, T, seed=0):
    """keys of n elements of key_bytes; T = the tile of the configuration they are meant for"""
    rng = np.random.default_rng([seed, n, key_bytes, PATTERNS.index(pattern)])
    dt = _udtype(key_bytes)
    bits = 8 * key_bytes
    ones = dt(_mask(bits))
    if pattern == "uniform":                       # (a) the full key width, top bit included
        return _rand_bits(rng, n, key_bytes)
    if pattern == "ones":                          # (b) real digit 255 shares its counter with the padding, in every pass
        return np.full(n, ones, dtype=dt)
    if pattern == "ones_sparse":                   # (c) ... except about 1 % of the keys
        k = np.full(n, ones, dtype=dt)
        pick = rng.random(n) < 0.01
        if n > 1:
            pick[rng.integers(0, n)] = True
        k[pick] = _rand_bits(rng, int(pick.sum()), key_bytes)
        return k
    if pattern == "one_bit":                       # (d) two counters for a whole wave
        return rng.integers(0, 2, size=n, dtype=np.uint64).astype(dt)
    if pattern in ("ascending", "descending"):     # (e) one long digit run per tile in the top passes
        step = _mask(bits) // n
        k = (np.arange(n, dtype=np.uint64) * np.uint64(step)).astype(dt)
        return k if pattern == "ascending" else k[::-1].copy()
    if pattern == "last_tile_ones":                # the padding rule's own edge: the last tile's real keys are all digit 255
        k = _rand_bits(rng, n, key_bytes)
        k[(n - 1) // T * T:] = ones
        return k
    raise ValueError(pattern)


def bit_range_case(n, key_bytes, begin, end, seed=0):
    """keys whose sort field [begin, end) ties often (n / 4 distinct values at most) under random bits outside it"""
    rng = np.random.default_rng([seed, n, begin, end])
    dt = _udtype(key_bytes)
    width = end - begin
    pool = rng.integers(0, 1 << 64, size=max(1, n // 4), dtype=np.uint64) & np.uint64(_mask(width))
    field = pool[rng.integers(0, len(pool), size=n)]
    outside = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) & np.uint64(M64 ^ (_mask(width) << begin))
    keys = ((field << np.uint64(begin)) | outside) & np.uint64(_mask(8 * key_bytes))
    return {"edge": f"bits [{begin}, {end}) of {8 * key_bytes}, ties under live bits outside", "keys": keys.astype(dt),
            "begin": begin, "end": end}


SKIP_CASES = ("first_constant", "middle_constant", "last_constant", "all_equal", "single")


def skip_case(name, n, key_bytes, seed=0):
    """full-width keys with one byte digit (or all of them) constant"""
    rng = np.random.default_rng([seed, n, key_bytes, SKIP_CASES.index(name)])
    dt = _udtype(key_bytes)
    npass = key_bytes
    if name == "single":
        n = 1
    keys = _rand_bits(rng, n, key_bytes)
    const = {"first_constant": [0], "middle_constant": [npass // 2], "last_constant": [npass - 1], "all_equal": list(range(npass)),
             "single": []}[name]
    for p in const:
        keys = (keys & dt(_mask(8 * key_bytes) ^ (0xFF << (8 * p)))) | dt(0xA5 << (8 * p))
    return {"edge": name, "keys": keys, "begin": 0, "end": 8 * key_bytes, "constant_passes": const}


def executed_passes_case(n, k, seed=0):
    """64-bit keys whose low 8 k bits are random (k executed passes) under random bits above the range"""
    rng = np.random.default_rng([seed, n, k])
    return {"edge": f"{k} executed passes", "keys": _rand_bits(rng, n, 8), "begin": 0, "end": 8 * k}


def split_case(n, val_bytes, aux_bytes, hi_bits, lead, pattern, T, seed=0):
    """split records: keys by `pattern` ("uniform", "ones", "one_bit"), random auxiliary words (the carried bytes included)"""
    rng = np.random.default_rng([seed, n, aux_bytes, hi_bits, lead])
    k32 = pattern_keys(pattern, n, 4, T, seed)
    if pattern == "ones":
        aux = np.full(n, _mask(8 * aux_bytes), dtype=_udtype(aux_bytes))
        if lead < aux_bytes:                                      # the carried bytes stay random
            aux = aux & _udtype(aux_bytes)(_mask(8 * lead)) | (_rand_bits(rng, n, aux_bytes) & _udtype(aux_bytes)(_mask(8 * aux_bytes) ^ _mask(8 * lead)))
    elif pattern == "one_bit":
        aux = _rand_bits(rng, n, aux_bytes) & _udtype(aux_bytes)((_mask(8 * aux_bytes) ^ _mask(8 * lead)) | 1)
    else:
        aux = _rand_bits(rng, n, aux_bytes)
    return {"edge": f"split v{val_bytes} w{aux_bytes} hi_bits {hi_bits} lead {lead} {pattern}", "keys": k32,
            "aux": aux.astype(_udtype(aux_bytes)), "hi_bits": hi_bits, "lead": lead}


EPOCH_PASSES = (8, 7, 5)


def _fill(total):
    """sorts of 8, 7 and 5 passes with `total` passes together, all three kinds present"""
    seq = [7, 5]
    rest = total - 12
    while rest % 8:
        seq.append(5)
        rest -= 5
    assert rest >= 0
    return seq + [8] * (rest // 8)


def epoch_sequence():
    """pass counts of the sorts of the epoch test: the tags wrap at executed pass 256, 511 and 766 of a fresh workspace — the first
    pass of a sort, a middle pass of a sort and the last pass of a sort"""
    seq = _fill(255) + [8]                 # passes 256..263: the wrap is this sort's first pass
    seq += _fill(508 - sum(seq)) + [8]     # passes 509..516: the wrap (511) is its third pass
    seq += _fill(766 - 7 - sum(seq)) + [7]  # passes 760..766: the wrap is its last pass
    return seq + [5, 8]


def epoch_wraps(seq):
    """[(sort index, position of the wrapping pass inside the sort: "first" / "middle" / "last")] and the epoch after every sort"""
    epoch, wraps, after = 0, [], []
    for i, k in enumerate(seq):
        epoch, at = epoch_after(epoch, k)
        if at is not None:
            wraps.append((i, "first" if at == 0 else ("last" if at == k - 1 else "middle")))
        after.append(epoch)
    return wraps, after
