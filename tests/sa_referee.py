"""A CPU referee for the suffix-array verifiers (verify.hip), and the corpora that drive them to their edges.

Plain Python / numpy, written from the rules in the comments above RefOrderCtx and from tests/ref_model.py; it shares no
code with verify.hip.  Test infrastructure (a helper module, not a conftest).

For every adjacent pair (i - 1, i) of an entry array the referee finds the length l of the common prefix of the two
suffixes and files the pair under exactly one kind:

  TIE     both suffixes end at l          -> right iff doc(i - 1) < doc(i)                  (canonical tie order)
  PREFIX  exactly one ends at l           -> right iff the shorter one comes first
  SAME    next bytes of one sign class    -> right iff they ascend
  MIXED   one byte >= 0x80, one < 0x80    -> unsigned order: right iff they ascend;
                                             reference order: the byte >= 0x80 comes first iff MORE than `chuck`
                                             suffixes share the l-byte prefix (a radix node of the reference)

The size of that bucket is the length of the maximal contiguous run of entries around the pair that have at least l
bytes and share them: defined on any array, damaged ones included.

Counts, named after what they referee:
  inversions, tie_violations, entry_sum, expected_entry_sum        cdb_debug_verify (plain unsigned order, no cap)
  ref_violations, mixed_pairs, node_pairs, tie_violations          cdb_debug_verify_reference (no cap)
  full_check_bad(plain)                                            sa_full_check_kernel: self_check(full) and the proof.
      A pair whose common prefix reaches `walk_cap` bytes without ending either suffix is not judged ("taken on trust
      beyond 4096"); chuck = 0 lets mixed pairs pass.
"""
import numpy as np

TIE, PREFIX, SAME, MIXED = 0, 1, 2, 3
M64 = (1 << 64) - 1


def pack_docs(docs):
    """(blob uint8[], doc_start uint64[ndocs + 1]) of a list of bytes objects"""
    ds = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=ds[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), ds


def _lcp(t, p, q, m):
    """length of the common prefix of t[p:p + m] and t[q:q + m]: slice compares in growing steps, then bisection"""
    k, step = 0, 16
    while k < m:
        e = min(m, k + step)
        if t[p + k:p + e] != t[q + k:q + e]:
            break
        k, step = e, step * 4
    else:
        return m
    lo, hi = k, e                                    # the first lo bytes agree, the first hi do not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if t[p + lo:p + mid] == t[q + lo:q + mid]:
            lo = mid
        else:
            hi = mid
    return lo


class Verdict:
    """what the referee found; per-pair arrays (index = position in `at`) for the corpus conditions"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def full_check_bad(self, plain, judge_mixed=True):
        """pairs sa_full_check_kernel must report: plain = the array claims unsigned order; judge_mixed=False is chuck = 0"""
        judged = ~self.trusted
        bad = (self.kind == TIE) & self.bad_tie | (self.kind == PREFIX) & self.bad_prefix | (self.kind == SAME) & self.descend
        if plain:
            bad |= (self.kind == MIXED) & self.descend
        elif judge_mixed:
            bad |= (self.kind == MIXED) & (self.high_first != self.node)
        return int(np.count_nonzero(bad & judged))


def judge(sa, blob, doc_start, bits, mask, chuck=None, walk_cap=None, only=None):
    """Referee every adjacent pair (i - 1, i) of `sa`, or the pairs i in `only`.  Every entry must name a real suffix.
    chuck defaults to the reference's max(4096, n // 256)."""
    t = bytes(blob) if not isinstance(blob, bytes) else blob
    ds = [int(x) for x in doc_start] if len(doc_start) < (1 << 16) else np.asarray(doc_start, dtype=np.int64)
    n = len(sa)
    bits, mask = int(bits), int(mask)
    if chuck is None:
        chuck = max(4096, n // 256)
    at = list(range(1, n)) if only is None else [int(i) for i in only]
    assert all(0 < i < n for i in at)

    def suffix(i):
        e = int(sa[i])
        d, o = e & mask, e >> bits
        assert d + 1 < len(ds) and o < int(ds[d + 1]) - int(ds[d]), ("entry names no suffix", i, e)
        p = int(ds[d]) + o
        return p, int(ds[d + 1]) - p, d

    def shares(i, pre):
        p, ln, _ = suffix(i)
        return ln >= len(pre) and t[p:p + len(pre)] == pre

    m = len(at)
    kind = np.zeros(m, dtype=np.int8)
    lcp = np.zeros(m, dtype=np.int64)
    short = np.zeros(m, dtype=np.int64)              # length of the shorter suffix
    descend = np.zeros(m, dtype=bool)                # SAME / MIXED: next byte of i - 1 > next byte of i
    bad_prefix = np.zeros(m, dtype=bool)
    bad_tie = np.zeros(m, dtype=bool)
    high_first = np.zeros(m, dtype=bool)
    node = np.zeros(m, dtype=bool)
    run = np.zeros(m, dtype=np.int64)                # MIXED: bucket size, counted up to chuck + 1 ...
    run_lo = np.zeros(m, dtype=np.int64)             # ... and the entries [run_lo, run_hi) counted
    run_hi = np.zeros(m, dtype=np.int64)
    for j, i in enumerate(at):
        pa, la, da = suffix(i - 1)
        pb, lb, db = suffix(i)
        lim = min(la, lb)
        l = _lcp(t, pa, pb, lim)
        lcp[j], short[j] = l, lim
        if l == la and l == lb:
            kind[j], bad_tie[j] = TIE, da >= db
        elif l == lim:
            kind[j], bad_prefix[j] = PREFIX, la > lb
        else:
            x, y = t[pa + l], t[pb + l]
            descend[j] = x > y
            if (x >= 0x80) == (y >= 0x80):
                kind[j] = SAME
            else:
                kind[j], high_first[j] = MIXED, x >= 0x80
                pre = t[pa:pa + l]
                cnt, k = 2, i - 2
                while cnt <= chuck and k >= 0 and shares(k, pre):
                    cnt, k = cnt + 1, k - 1
                run_lo[j] = k + 1
                k = i + 1
                while cnt <= chuck and k < n and shares(k, pre):
                    cnt, k = cnt + 1, k + 1
                run_hi[j] = k
                run[j], node[j] = cnt, cnt > chuck
    mixed = kind == MIXED
    v = Verdict(at=np.asarray(at, dtype=np.int64), kind=kind, lcp=lcp, short=short, descend=descend, bad_prefix=bad_prefix,
                bad_tie=bad_tie, high_first=high_first, node=node, run=run, run_lo=run_lo, run_hi=run_hi, n=n, chuck=chuck, walk_cap=walk_cap,
                trusted=np.zeros(m, dtype=bool) if walk_cap is None else (lcp >= walk_cap) & (short > walk_cap))
    v.inversions = int(np.count_nonzero(bad_prefix | ((kind == SAME) | mixed) & descend))
    v.tie_violations = int(np.count_nonzero(bad_tie))
    v.ref_violations = int(np.count_nonzero(bad_prefix | (kind == SAME) & descend | mixed & (high_first != node)))
    v.mixed_pairs = int(np.count_nonzero(mixed))
    v.node_pairs = int(np.count_nonzero(mixed & node))
    if only is None:
        v.entry_sum = int(np.asarray(sa, dtype=np.uint64).sum(dtype=np.uint64)) if n else 0
        total = 0
        for d in range(len(ds) - 1):
            ln = int(ds[d + 1]) - int(ds[d])
            total += ((ln * (ln - 1) // 2) << bits) + ln * d
        v.expected_entry_sum = total & M64
    return v


def suffix_bytes(sa, blob, doc_start, bits, mask, i):
    """the suffix entry i names"""
    e = int(sa[i])
    d = e & int(mask)
    return bytes(blob[int(doc_start[d]) + (e >> int(bits)):int(doc_start[d + 1])])


def mixed_edge_pairs(v):
    """(i, j): mixed pairs judged as leaves whose bucket starts at entry 0 / ends at entry n - 1 (None where there is none)"""
    leaf = (v.kind == MIXED) & ~v.node
    first = v.at[leaf & (v.run_lo == 0)]
    last = v.at[leaf & (v.run_hi == v.n)]
    return (int(first[0]) if len(first) else None), (int(last[0]) if len(last) else None)


def long_pairs(v):
    """the pairs of long_docs() at the walk limit, by name -> i (each exists once)"""
    out = {}
    for name, sel in (("lcp4095", (v.lcp == 4095) & (v.kind == SAME)),
                      ("lcp4096_longer", (v.lcp == 4096) & (v.short > 4096) & (v.kind == SAME)),
                      ("lcp4096_ends", (v.lcp == 4096) & (v.short == 4096) & (v.kind == PREFIX))):
        at = v.at[sel]
        assert len(at) == 1, (name, at)
        out[name] = int(at[0])
    return out


def swap_pairs(sa, ks):
    """copy of sa with entries k and k + 1 exchanged for every k in ks, one exchange after the other"""
    out = np.array(sa, copy=True)
    ks = np.asarray(list(ks), dtype=np.int64)
    if len(ks) > 1 and np.all(np.diff(ks) > 1):       # disjoint pairs: at once
        out[ks], out[ks + 1] = out[ks + 1].copy(), out[ks].copy()
    else:
        for k in ks:
            out[k], out[k + 1] = out[k + 1], out[k]
    return out


def third(n, r):
    """the pairs (k, k + 1), k = r mod 3: three of these damage every adjacent pair once"""
    return range(r, n - 1, 3)


# ---- corpora -----------------------------------------------------------------------------------------------------
HEAD_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33)
_ALPHABET = (0x00, 0x01, 0x61, 0x62)


def _draw(rs, n, alphabet=_ALPHABET):
    return bytes(alphabet[i] for i in rs.randint(0, len(alphabet), n))


def heads_docs(seed=1):
    """Suffixes that first differ, end, or tie at every length 0..33 — inside, at the edge of and behind the 16-byte head
    sa_full_check_kernel compares first — over an alphabet with real 0x00 bytes (its padding behind a suffix's end)."""
    rs = np.random.RandomState(seed)
    docs = []
    for L in HEAD_LENGTHS:
        P = _draw(rs, L)
        docs += [P + b"\x00", P + b"\x01", P + b"a", P, P + b"a", P + b"\x00\x00", P + b"a\x00\x00\x00"]
    docs += [_draw(rs, int(ln)) for ln in rs.randint(0, 41, 150)]
    docs = [docs[i] for i in rs.permutation(len(docs))]
    # the text ends in a short document: the 16-byte window of its suffixes runs past the end of the text
    last = next(i for i in range(len(docs) - 1, -1, -1) if 0 < len(docs[i]) < 16)
    docs.append(docs.pop(last))
    return docs


def heads8_docs(seed=1):
    """heads with 8-byte entries: 2^16 empty documents (17 document bits) and one of 32 769 bytes (16 offset bits)"""
    rs = np.random.RandomState(seed + 100)
    return [b""] * (1 << 15) + heads_docs(seed) + [_draw(rs, 32769)] + [b""] * (1 << 15)


def mixed_docs(extra):
    """Reference order at its threshold (chuck = 4096): the bucket of 'q' holds 4096 + extra suffixes whose next bytes
    lie on both sides of 0x80 — a sorted leaf at 4096, a radix node (bytes >= 0x80 first) at 4097.  The bucket of 'r'
    (mixed, a leaf) ends the array; the bucket of 0x80 (mixed, a leaf) starts it."""
    assert extra in (0, 1)
    docs = []
    for i in range(4096 + extra):
        docs.append(b"q" + (bytes([0x41 + (i // 2) % 16]) if i % 2 == 0 else bytes([0xC3, 0x80 + (i // 2) % 16])))
    docs += [b"r" + (b"B" if i % 2 == 0 else b"\xC3\xA0") for i in range(50)]
    # 0x80 is the smallest byte >= 0x80: in the root node's signed child order its bucket comes first
    docs += [b"\x80" + (b"C" if i % 2 == 0 else b"\xC3\xA1") for i in range(6)]
    # a suffix that is a prefix of its neighbour, whose next byte is >= 0x80: a prefix, not a mixed pair (the zero
    # padding behind the end of a 16-byte head is no byte of the suffix)
    docs += [b"\xC3"] * 3
    return docs


def long_docs(seed=5):
    """Common prefixes at the 4096-byte limit of the full sweep's walk: 4095, 4096 with both suffixes longer, 4096 with the
    shorter one ending there.  Returns (docs, k): document 3 is D[k:k + 4096]."""
    rs = np.random.RandomState(seed)
    alphabet = tuple(range(0x61, 0x6B))
    D = _draw(rs, 5200, alphabet)
    x = bytes([0x6A if D[4500] != 0x6A else 0x69])
    E = D[:4500] + x + _draw(rs, 699, alphabet)
    k = next(k for k in range(300, 600) if D[k + 4096] != 0x61)
    docs = [D, D, E, D[k:k + 4096]] + [_draw(rs, int(ln), alphabet) for ln in rs.randint(0, 41, 200)]
    return docs, k


def seam_corpus():
    """2^24 + 2^16 suffixes, 4-byte entries: the grid-stride wraps of the full sweep and the proof's slice seam"""
    from coffeedb_amd import workloads as W
    want = (1 << 24) + (1 << 16)
    lens = W.random_bytes(170_000, 41, 1, 200).astype(np.uint64)
    ds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nd = int(np.searchsorted(ds, want, side="left"))  # first document boundary at or past `want`
    ds = ds[:nd + 1].copy()
    ds[nd] = want                                     # the last document is cut to fit
    assert ds[nd] > ds[nd - 1]
    return W.random_bytes(want, 42, 0x61, 0x6A), ds
