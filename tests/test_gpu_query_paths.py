"""The three row builders of the batched query (query.hip: query_typed) in sequence and at their hit-count edges.

Which builder answers a batch depends on what the previous batch on the handle did: a wavefront-path batch arms the next one to
run speculatively in buffers of cap = max(1.5 H_prev, 4096) hits; a hit list over 64 or a list ending beyond cap raises a device
flag and the batch is redone with the totals known (wavefront path if every list has <= 64 hits, else expand + radix sort, cut
into chunks under query_hit_budget).  Every step here is checked twice: the full result against a brute force over the documents'
own bytes (bytes.find; no suffix array, no oracle), and the deltas of the per-handle path counters (cdb_get_stat "query_*_batches")
against a few-line restatement of the dispatch rule fed with the brute force's own hit counts.  Nothing is read back from the
library to form an expectation.

The corpora PLANT their hit counts: token T_h occurs exactly h times for h in HS, all in one document / one per document / in
mixed runs.  The CPU tests of this file (not marked gpu) tie the brute force to the oracle and show that the seeded fuzz reaches
every path."""
import bisect
import os
import threading

import numpy as np
import pytest

HS = (1, 2, 63, 64, 65, 66, 128, 4095, 4096, 4097)
SMALL_HS = (1, 2, 63, 64, 65)                 # the corpus below 4096 suffixes
TOKEN_LEN = {4097: 3, 4096: 4, 4095: 5, 128: 6, 66: 7, 65: 8, 64: 9, 63: 10, 2: 11, 1: 12}   # distinct lengths 3..12
STATS = ("batches", "spec", "spills", "wave", "sort", "chunks", "empty")
STAT_NAMES = {"batches": "query_batches", "spec": "query_spec_batches", "spills": "query_spec_spills", "wave": "query_wave_batches",
              "sort": "query_sort_batches", "chunks": "query_sort_chunks", "empty": "query_empty_batches"}
FUZZ_N = int(os.environ.get("CDB_FUZZ_PATHS_N", "30"))
FUZZ_BASE = 4100                               # seeds FUZZ_BASE .. FUZZ_BASE + 29: test_fuzz_plans_reach_every_path states what they reach


# ---------------------------------------------------------------------------------------------------------------- brute force
class Corpus:
    """Documents, ids and the brute-force answers over them."""

    def __init__(self, docs, ids, tok=None, name=""):
        self.docs = list(docs)
        self.ids = np.asarray(ids, dtype=np.int64)
        self.tok = dict(tok or {})
        self.name = name
        self.text = b"".join(self.docs)
        self.ds = np.zeros(len(self.docs) + 1, dtype=np.uint64)
        np.cumsum([len(d) for d in self.docs], out=self.ds[1:])
        self._starts = self.ds[:-1].tolist()
        self.blob = np.frombuffer(self.text, dtype=np.uint8)
        self._cache = {}
        self._pool = None

    def occ(self, kw):
        """[(document index, [offsets of every (overlapping) occurrence inside the document, ascending])], ascending document."""
        r = self._cache.get(kw)
        if r is None:
            # only a document that holds the START of an occurrence in the joined text can hold one of its own: those are the
            # candidates; the answer itself comes from bytes.find over each candidate's own bytes (a match of the joined text
            # that runs over a document boundary finds nothing there)
            cand, i = [], self.text.find(kw)
            while i >= 0:
                d = bisect.bisect_right(self._starts, i) - 1
                if not cand or cand[-1] != d:
                    cand.append(d)
                i = self.text.find(kw, i + 1)
            r = []
            for d in cand:
                doc, offs = self.docs[d], []
                i = doc.find(kw)
                while i >= 0:
                    offs.append(i)
                    i = doc.find(kw, i + 1)
                if offs:
                    r.append((d, offs))
            self._cache[kw] = r
        return r

    def hits(self, kw):
        return sum(len(o) for _, o in self.occ(kw))

    def rows(self, kw):
        return [(int(self.ids[d]), len(o)) for d, o in self.occ(kw)]

    def expect(self, kws):
        """(row_ptr, ids, counts, hits, hit_ptr, offsets) of a batch, as index.cpp:316-322 orders them."""
        rp, ids, cnt, off = [0], [], [], []
        for kw in kws:
            o = self.occ(kw)
            ids.extend(int(self.ids[d]) for d, _ in o)
            cnt.extend(len(x) for _, x in o)
            for _, x in o:
                off.extend(x)
            rp.append(len(ids))
        cnt = np.asarray(cnt, dtype=np.int64)
        hp = np.zeros(len(cnt) + 1, dtype=np.uint64)
        np.cumsum(cnt, out=hp[1:])
        return (np.asarray(rp, dtype=np.uint64), np.asarray(ids, dtype=np.int64), cnt, int(cnt.sum()), hp, np.asarray(off, dtype=np.uint64))

    def pool(self):
        """keywords with 1..64 hits (lowercase substrings of the text, seeded) — the filling of wavefront-class batches"""
        if self._pool is None:
            rng = np.random.default_rng(99)
            out, seen = [], set()
            for _ in range(4000):
                if len(out) == 320:
                    break
                i = int(rng.integers(len(self.text)))
                d = bisect.bisect_right(self._starts, i) - 1
                a, ln = i - self._starts[d], int(rng.integers(6, 10))
                kw = self.docs[d][a:a + ln]
                if len(kw) < ln:
                    continue
                if kw in seen or not _lower(kw) or not 1 <= self.hits(kw) <= 64:
                    continue
                seen.add(kw)
                out.append(kw)
            assert len(out) >= 40, (self.name, len(out))
            self._pool = out
        return self._pool

    def with_doc(self, id_, doc):
        return Corpus(self.docs + [doc], np.append(self.ids, id_), self.tok, self.name + "+1")


MISSES = (b"ZZZ", b"QX", b"abcdabcdabcdabcdabcdabcdabcd", b"!", b"dddddddddddddddddddddddddddddddddz", b"BZ", b"~~")


def _draw_tokens(rng, hs):
    while True:
        tok = {h: bytes(rng.choice(list(b"BCDEFG"), size=TOKEN_LEN[h]).astype(np.uint8)) for h in hs}
        v = list(tok.values())
        if not any(a != b and a in b for a in v for b in v):   # no token inside another: the planted counts are the counts
            return tok


def _filler(rng, n):
    return rng.integers(0x61, 0x65, size=n).astype(np.uint8).tobytes()


def _put_inside_filler(rng, doc, piece):
    """`piece` over the middle of a stretch of lowercase filler"""
    for _ in range(8):
        a = int(rng.integers(4, len(doc) - 6))
        if _lower(doc[a - 4:a + 6]):
            return doc[:a] + piece + doc[a + len(piece):]
    return doc


def _lower(b):
    return all(0x61 <= x <= 0x64 for x in b)


def make_corpus(kind):
    """kind: one_doc / per_doc / mixed (4-byte entries, documents of 20..200 bytes plus what is planted in them), wide (8-byte
    entries: one 150 000-byte document among 16 500 tiny ones), high (bytes >= 0x80 in the filler), small (below 4096 suffixes:
    the reference search)."""
    layout = kind if kind in ("one_doc", "per_doc", "mixed") else "mixed"
    rng = np.random.default_rng({"one_doc": 11, "per_doc": 12, "mixed": 13, "wide": 14, "high": 15, "small": 16}[kind])
    hs = SMALL_HS if kind == "small" else HS
    tok = _draw_tokens(rng, hs)
    nd = {"one_doc": 1200, "per_doc": 4400, "mixed": 1200, "wide": 16500, "high": 1200, "small": 24}[kind]
    items = [[] for _ in range(nd)]                            # tokens planted per document
    for h in hs:
        if layout == "one_doc":
            items[int(rng.integers(nd))].extend([tok[h]] * h)
        elif layout == "per_doc":
            for d in rng.choice(nd, size=h, replace=False):
                items[int(d)].append(tok[h])
        else:                                                  # runs of 1..9 (long lists: 1..40) in random documents, some met twice
            left = h
            while left:
                r = min(left, int(rng.integers(1, 41 if h > 128 else 10)))
                items[int(rng.integers(nd))].extend([tok[h]] * r)
                left -= r
    runs = [[] for _ in range(nd)]                             # the self-overlapping token: AAA inside runs of A
    for d, rl in ((0, (3,)), (nd // 3, (4, 10)), (nd // 2, (40,)), (nd - 1, (5, 2, 9))):
        runs[d].extend(rl)
    docs = []
    for d in range(nd):
        parts = [bytes(t) for t in items[d]] + [b"A" * r for r in runs[d]]
        order = rng.permutation(len(parts))
        if kind == "small":
            flen = int(rng.integers(20, 60))
        elif layout == "per_doc":
            flen = int(rng.integers(20, 201)) if d % 12 == 0 else int(rng.integers(20, 44))
        elif kind == "wide":                                   # 2^14 < documents and 2^17 < the longest: 15 + 18 bits, 8-byte entries;
            flen = int(rng.integers(1, 4))                     # under 256 KiB of text that leaves a few bytes per document
        else:
            flen = int(rng.integers(20, 201))
        flen = max(flen, len(parts) + 1)
        if kind == "wide" and d == nd // 2 + 1:
            flen = 150_000
        fill = _filler(rng, flen)
        cuts = np.sort(rng.choice(np.arange(1, flen), size=len(parts), replace=False)) if parts else []
        out, prev = [], 0
        for c, k in zip(cuts, order):                          # every planted piece has lowercase filler on both sides
            out += [fill[prev:int(c)], parts[int(k)]]
            prev = int(c)
        out.append(fill[prev:])
        docs.append(b"".join(out))
        # a few two-byte UTF-8 sequences (bytes >= 0x80).  With reference_compat the reference's array holds their suffixes in FRONT
        # (signed order) while its bisection compares unsigned, so the smallest keyword range of the text would swallow them
        # (SURVEY Q2); some blanks give the text a smaller byte than any keyword's, and the answers are the true ones — which
        # test_brute_force_is_the_oracle shows for every keyword used on this corpus
        if kind == "high" and d % 50 == 7:
            docs[-1] = _put_inside_filler(rng, docs[-1], b"\xc3\xa9")
        if kind == "high" and d % 5 == 3:
            docs[-1] = _put_inside_filler(rng, docs[-1], b" ")
    ids = rng.permutation(nd).astype(np.int64) * 7 - 3 * nd    # shuffled, partly negative, affine
    return Corpus(docs, ids, tok, kind)


_CORPORA = {}


def corpus_of(kind):
    if kind not in _CORPORA:
        _CORPORA[kind] = make_corpus(kind)
    return _CORPORA[kind]


# ------------------------------------------------------------------------------------------------- the dispatch rule, restated
class Model:
    """query.hip's choice of row builder from (with_offsets, the hit counts, the previous step's cap)."""

    def __init__(self):
        self.cap = 0                      # > 0: the next batch runs speculatively in buffers for `cap` hits
        self.wave_rows = True
        self.budget = 1 << 31

    def predict(self, hits, with_offsets=False):
        d = dict.fromkeys(STATS, 0)
        d["batches"] = 1
        d["cause"] = None
        if not hits:
            d["empty"] = 1
            return d
        H, maxh = sum(hits), max(hits)
        if not with_offsets and self.wave_rows and self.cap > 0:
            d["spec"] = 1
            off, long_, over = 0, False, False
            for h in hits:
                long_ |= h > 64
                over |= off + h > self.cap
                off += h
            if not (long_ or over):
                self.cap = max(H + H // 2, 4096)
                return d
            d["spills"], d["cause"] = 1, "long" if long_ else "cap"
            self.cap = 0
        if H == 0:
            d["empty"] = 1                # (cap stays what it is)
            return d
        if not with_offsets and maxh <= 64 and self.wave_rows and H <= 1 << 28:
            d["wave"] = 1
            self.cap = max(H + H // 2, 4096)
            return d
        self.cap = 0
        d["sort"], d["chunks"] = 1, 1
        if H > self.budget:               # cut in front of the pattern that overflows the budget (a lone pattern is never cut)
            hoff = np.concatenate([[0], np.cumsum(hits)]).tolist()
            cuts, start = 0, 0
            for j in range(1, len(hits) + 1):
                if hoff[j] - hoff[start] > self.budget and j - 1 > start:
                    cuts += 1
                    start = j - 1
            d["chunks"] = cuts + 1
        return d

    def rebuilt(self):                    # builds, loads and proof repairs disarm
        self.cap = 0


def _pack(kws):
    blob = np.frombuffer(b"".join(kws), dtype=np.uint8)
    offs = np.zeros(len(kws) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in kws], out=offs[1:])
    return blob, offs


class Runner:
    """One index (or a sharded one) with the brute force and the model beside it; every query goes through here."""

    def __init__(self, target, corpus, parts=None):
        self.t = target
        self.c = corpus
        self.parts = parts or [(target, corpus, Model())]      # (handle with the counters, its documents, its model)

    def snap(self):
        return [{k: int(g.stat(STAT_NAMES[k])) for k in STATS} for g, _, _ in self.parts]

    def _check_delta(self, before, preds, what):
        after = self.snap()
        for i, (b, a, p) in enumerate(zip(before, after, preds)):
            got = {k: a[k] - b[k] for k in STATS}
            assert got == {k: p[k] for k in STATS}, (what, "part", i, "got", got, "predicted", p)

    def batch(self, kws, offsets=False, device=False, what=""):
        want = self.c.expect(kws)
        preds = [m.predict([c.hits(k) for k in kws], offsets) for _, c, m in self.parts]
        before = self.snap()
        blob, offs = _pack(kws)
        if device:
            got = _device_batch(self.t, blob, offs)
        elif offsets:
            got = self.t.query_batch_offsets(blob, offs)
        else:
            got = self.t.query_batch(blob, offs)
        info = (self.c.name, what, len(kws), "offsets" if offsets else "", "device" if device else "")
        assert np.array_equal(got[0], want[0]), info + ("row_ptr",)
        assert np.array_equal(got[1], want[1]), info + ("ids",)
        assert np.array_equal(got[2], want[2]), info + ("counts",)
        if offsets:
            assert np.array_equal(got[3], want[4]) and np.array_equal(got[4], want[5]), info + ("offsets",)
        else:
            assert got[3] == want[3], info + ("hits", got[3], want[3])
        self._check_delta(before, preds, info)
        return preds[0]

    def lone(self, kw, what=""):
        (g, c, m), = self.parts
        h = c.hits(kw)
        # up to 4096 hits the lone-keyword kernels answer (no batch at all); a longer list is handed to the batch path
        pred = m.predict([h]) if h > 4096 or len(kw) > 120 else dict.fromkeys(STATS, 0)
        before = self.snap()
        got = self.t.query(kw)
        assert got == c.rows(kw), (c.name, what, kw, h, got[:3])
        self._check_delta(before, [pred], (c.name, what, kw, h))
        return pred

    def reset(self):
        """a known state whatever ran before: a batch with occurrence offsets and at least one hit never arms and always disarms"""
        kw = self.c.tok[max(self.c.tok)]
        assert all(c.hits(kw) > 0 for _, c, _ in self.parts)
        blob, offs = _pack([kw])
        self.t.query_batch_offsets(blob, offs)
        for _, _, m in self.parts:
            m.cap = 0

    def arm(self, kws=None):
        self.reset()
        p = self.batch(kws or [self.c.tok[1], self.c.tok[2]] + self.c.pool()[:6], what="arm")
        assert p["wave"] == 1 and all(m.cap >= 4096 for _, _, m in self.parts[:1])
        return p

    def set_option(self, name, value):
        self.t.set_option(name, value)
        for _, _, m in self.parts:
            if name == "wave_rows":
                m.wave_rows = bool(value)
            if name == "query_hit_budget":
                m.budget = min(value, 1 << 31) if value > 0 else 1


def _device_batch(g, blob, offs):
    import torch
    d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(16, dtype=np.uint8)])).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    npat = len(offs) - 1
    r = g.query_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), npat, len(blob))

    def dev(ptr, cnt):
        if cnt == 0:
            return np.empty(0, dtype=np.int64)

        class A:
            __cuda_array_interface__ = {"shape": (int(cnt),), "typestr": "<i8", "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(A(), device="cuda").cpu().numpy().copy()
    nrows = int(r.nrows)
    return dev(r.d_row_ptr, npat + 1).astype(np.uint64), dev(r.d_ids, nrows), dev(r.d_counts, nrows), int(r.nhits)


def exact_total(c, total, first=None):
    """a batch whose every hit list has <= 64 entries and whose hits sum to `total` exactly (in the documents of `c`)"""
    coins = sorted({c.hits(k): k for k in [c.tok[64], c.tok[63], c.tok[2], c.tok[1]] + c.pool() if 1 <= c.hits(k) <= 64}.items(), reverse=True)
    assert coins[-1][0] == 1, "a keyword with one hit is needed"
    out, left = ([first] if first else []), total - (c.hits(first) if first else 0)
    for h, k in coins:
        out += [k] * (left // h)
        left %= h
    assert sum(c.hits(k) for k in out) == total and max(c.hits(k) for k in out) <= 64
    return out


def fits_batch(c, n, seed):
    """n keywords of the wavefront class: pool substrings, the planted tokens up to 64 hits, a few misses"""
    rng = np.random.default_rng(seed)
    src = c.pool() + [c.tok[1], c.tok[2], c.tok[63], c.tok[64], b"AAA", b"AAAA", MISSES[0], MISSES[2]]
    return [src[int(i)] for i in rng.integers(len(src), size=n)]


# ------------------------------------------------------------------------------------------------------ sequences (a) .. (c)
def seq_a(r):
    c = r.c
    r.reset()
    p = r.batch([c.tok[1], c.tok[2], c.tok[63], c.tok[64], b"AAA"] + c.pool()[:20], what="a1")
    assert (p["wave"], p["spec"]) == (1, 0)
    p = r.batch(fits_batch(c, 60, 1), what="a2")
    if len(r.parts) == 1:
        assert (p["spec"], p["spills"]) == (1, 0), p


def seq_b(r, where, long_h):
    c = r.c
    base = fits_batch(c, 300, 2)
    r.arm(base[::-1])                                            # (cap = 1.5 x this batch's own hits: only the long list can spill)
    at = {"first": 0, "middle": 150, "last": 300}[where]
    kws = base[:at] + [c.tok[long_h]] + base[at:]
    p = r.batch(kws, what=f"b {where} {long_h}")
    if len(r.parts) == 1:
        want = (1, 1, 1, "long") if long_h > 64 else (1, 0, 0, None)
        assert (p["spec"], p["spills"], p["sort"], p["cause"]) == want, p
    p = r.batch(base, what="b next")
    if len(r.parts) == 1:
        assert p["spec"] == (0 if long_h > 64 else 1), p


def seq_c(r):
    c0 = r.parts[0][1]                                           # (totals are placed on the first part's own documents)
    one = [k for k in [c0.tok[1]] + c0.pool() if c0.hits(k) == 1][:1]
    for total, spill in ((4096, False), (4097, True), (8000, True)):
        r.arm(one)                                               # H_prev = 1: cap at its floor of 4096
        assert r.parts[0][2].cap == 4096
        p = r.batch(exact_total(c0, total), what=f"c floor {total}")
        assert (p["spec"], p["spills"], p["cause"], p["wave"]) == (1, int(spill), "cap" if spill else None, int(spill)), p
    for extra in (0, 1):                                         # above the floor: H_prev = 10 000 -> cap = 15 000
        r.arm(exact_total(c0, 10_000))
        assert r.parts[0][2].cap == 15_000
        p = r.batch(exact_total(c0, 15_000 + extra, first=one[0] if extra else None), what=f"c cap+{extra}")
        assert (p["spec"], p["spills"], p["cause"]) == (1, extra, "cap" if extra else None), p
        p = r.batch(exact_total(c0, 15_000 + extra)[::-1], what="c next")   # (the short lists first this time)
        assert p["spec"] == 1


# ------------------------------------------------------------------------------------------------------------------ fuzz plan
FUZZ_KINDS = ("wave", "long", "capacity", "miss", "offsets", "rebuild")


def fuzz_plan(c, seed):
    """8 steps of (kind, keywords, budget) and what the model predicts for each — computed without a GPU"""
    rng = np.random.default_rng(FUZZ_BASE + seed)
    m = Model()
    m.budget = int(rng.choice([700, 1 << 31]))
    steps = []
    for _ in range(8):
        kind = FUZZ_KINDS[int(rng.choice(6, p=[0.3, 0.2, 0.2, 0.08, 0.12, 0.1]))]
        n = int(rng.integers(1, 601))
        if kind == "rebuild":
            m.rebuilt()
            steps.append((kind, [], None))
            continue
        if kind == "wave":
            kws = fits_batch(c, min(n, 200), int(rng.integers(1 << 30)))
        elif kind == "long":
            kws = fits_batch(c, n, int(rng.integers(1 << 30)))
            kws.insert(int(rng.integers(len(kws) + 1)), c.tok[int(rng.choice([65, 66, 128, 4095, 4097]))])
        elif kind == "capacity":                                  # every list <= 64, one hit more than an armed handle holds
            kws = exact_total(c, min(max(m.cap, 4096) + 1, 600 * 60))
            rng.shuffle(kws)
        elif kind == "miss":
            kws = [MISSES[int(i)] for i in rng.integers(len(MISSES), size=n)]
        else:
            kws = fits_batch(c, min(n, 120), int(rng.integers(1 << 30))) + [c.tok[65]]
        assert 1 <= len(kws) <= 601
        steps.append((kind, kws, m.predict([c.hits(k) for k in kws], kind == "offsets")))
    return m.budget, steps


# ------------------------------------------------------------------------------------------------------------- CPU-only tests
def test_planted_counts_and_shapes():
    for kind in ("one_doc", "per_doc", "mixed", "wide", "high", "small"):
        c = corpus_of(kind)
        n = len(c.text)
        assert (n < 4096) if kind == "small" else (128 << 10) <= n <= (256 << 10), (kind, n)
        assert len(set(c.ids.tolist())) == len(c.ids) and (c.ids < 0).any() and (c.ids > 0).any()
        for h, t in c.tok.items():
            assert c.hits(t) == h, (kind, h, c.hits(t))
        assert c.hits(b"AAA") == 1 + 2 + 8 + 38 + 3 + 7 and c.hits(b"AAAA") == 1 + 7 + 37 + 2 + 6
        assert all(c.hits(k) == 0 for k in MISSES)
        if kind == "one_doc":
            assert all(len(c.occ(t)) == 1 for t in c.tok.values())
        if kind == "per_doc":
            assert all(len(c.occ(t)) == h for h, t in c.tok.items())
        if kind == "mixed":
            assert 1 < len(c.occ(c.tok[4096])) < 4096
        if kind == "wide":
            assert max(len(d) for d in c.docs) >= 150_000
        if kind == "high":
            assert 4 <= sum(b >= 0x80 for b in c.text) <= 400


@pytest.mark.parametrize("kind", ["mixed", "high", "small"])
def test_brute_force_is_the_oracle(kind):
    """The restatement above against OracleIndex (the reference's own search over its own suffix array): CSR, ids, counts, hits,
    and the occurrence offsets through the oracle's highlight spans (tokens do not overlap themselves: a span is an occurrence)."""
    from oracle import OracleIndex
    c = corpus_of(kind)
    o = OracleIndex()
    o.add_bulk(c.ids, c.blob, c.ds)
    o.build(2)
    o.canonicalize()
    kws = list(c.tok.values()) + [b"AAA", b"AAAA", b"AA", b"A"] + list(MISSES) + c.pool() + [c.tok[64]] * 3   # (every keyword the GPU tests send)
    got = c.expect(kws)
    want = o.query_batch(*_pack(kws))
    assert got[3] == want[3] and all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))
    for kw in list(c.tok.values()) + c.pool()[:5]:
        assert c.rows(kw) == o.query(kw)
    for kw in c.tok.values():                 # (planted with filler between them: no two occurrences touch)
        spans = o.highlight_spans([kw], c.ids)
        assert spans == [(int(c.ids[d]), [(a, a + len(kw) - 1) for a in offs]) for d, offs in c.occ(kw)]
    row = c.expect([c.tok[2], c.tok[1]])
    assert row[4].tolist() == [0] + np.cumsum(row[2]).tolist() and len(row[5]) == 3


def test_model_on_hand_made_cases():
    m = Model()
    assert m.predict([3, 64, 0])["wave"] == 1 and m.cap == 4096
    p = m.predict([64] * 64)
    assert (p["spec"], p["spills"]) == (1, 0) and m.cap == 6144
    m.cap = 4096
    p = m.predict([64] * 64 + [1])
    assert (p["spec"], p["spills"], p["cause"], p["wave"]) == (1, 1, "cap", 1) and m.cap == 6145
    p = m.predict([1, 65, 1])
    assert (p["spec"], p["spills"], p["cause"], p["sort"], p["chunks"]) == (1, 1, "long", 1, 1) and m.cap == 0
    assert m.predict([0, 0])["empty"] == 1 and m.predict([])["empty"] == 1
    m.budget = 100
    assert m.predict([60, 60, 60, 300, 1], True)["chunks"] == 5     # {60}, {60}, {60}, {300}, {1}: a chunk ends in front of the pattern that overflows it
    m.cap = 4096
    assert m.predict([0], True)["empty"] == 1 and m.cap == 4096


def test_fuzz_plans_reach_every_path():
    """Over the default 30 seeds the plans hold 35 speculative successes, 21 spills by a long list, 17 by capacity and 42 chunked
    sorts (counted here from the predictions alone)."""
    c = corpus_of("mixed")
    n = {"spec_ok": 0, "long": 0, "cap": 0, "chunked": 0}
    for seed in range(30):
        for _, _, p in fuzz_plan(c, seed)[1]:
            if p:
                n["spec_ok"] += p["spec"] - p["spills"]
                n["long"] += p["cause"] == "long"
                n["cap"] += p["cause"] == "cap"
                n["chunked"] += p["chunks"] > 1
    print("fuzz path counts over 30 seeds:", n)
    assert min(n.values()) >= 3, n


# ----------------------------------------------------------------------------------------------------------------- GPU tests
gpu = pytest.mark.gpu
FULL = ["one_doc", "per_doc", "mixed", "wide", "high", "high_plain"]
ALL = FULL + ["small"]
_HANDLES = {}


def _index(c, opts=()):
    from coffeedb_amd import capi
    g = capi.GpuStringIndex()
    for k, v in opts:
        g.set_option(k, v)
    g.add_bulk(c.ids, c.blob, c.ds)
    g.build()
    return g


@pytest.fixture(scope="module")
def runners():
    """one build per corpus, shared by the tests of this file (each starts from Runner.reset / Runner.arm)"""
    def get(kind):
        if kind not in _HANDLES:
            c = corpus_of("high" if kind == "high_plain" else kind)
            g = _index(c, (("reference_compat", 0),) if kind == "high_plain" else ())
            assert g.sa_width == (8 if kind == "wide" else 4)
            _HANDLES[kind] = Runner(g, c)
        return _HANDLES[kind]
    yield get
    for r in _HANDLES.values():
        r.t.close()
    _HANDLES.clear()


@gpu
@pytest.mark.parametrize("kind", ALL)
def test_a_wave_then_speculative(runners, kind):
    seq_a(runners(kind))


@gpu
@pytest.mark.parametrize("long_h", [65, 64])
@pytest.mark.parametrize("where", ["middle", "first", "last"])
@pytest.mark.parametrize("kind", ALL)
def test_b_one_long_list_among_300(runners, kind, where, long_h):
    seq_b(runners(kind), where, long_h)


@gpu
@pytest.mark.parametrize("kind", ALL)
def test_c_totals_at_cap_and_one_over(runners, kind):
    seq_c(runners(kind))


@gpu
@pytest.mark.parametrize("kind", ALL)
def test_d_all_miss_batches(runners, kind):
    r = runners(kind)
    r.arm()
    p = r.batch(list(MISSES) * 3, what="d armed")
    assert (p["spec"], p["spills"], p["empty"]) == (1, 0, 0) and r.parts[0][2].cap == 4096
    r.reset()
    p = r.batch(list(MISSES) * 3, what="d not armed")
    assert (p["spec"], p["empty"]) == (0, 1)
    p = r.batch(fits_batch(r.c, 50, 4), what="d normal")
    assert p["wave"] == 1


@gpu
@pytest.mark.parametrize("kind", ALL)
def test_e_offsets_batch_between(runners, kind):
    r = runners(kind)
    c = r.c
    r.arm()
    kws = fits_batch(c, 80, 5) + [c.tok[65], b"AAA", c.tok[max(c.tok)]]
    p = r.batch(kws, offsets=True, what="e offsets")
    assert (p["spec"], p["sort"]) == (0, 1)
    p = r.batch(fits_batch(c, 80, 6), what="e after")
    assert (p["spec"], p["wave"]) == (0, 1)
    r.arm()
    p = r.batch(list(MISSES), offsets=True, what="e offsets, no hit")   # (leaves the handle armed)
    assert p["empty"] == 1
    assert r.batch(fits_batch(c, 80, 7), what="e after no hit")["spec"] == 1


@gpu
def test_f_rebuild_load_and_repair_disarm(tmp_path):
    from coffeedb_amd import capi
    c = corpus_of("mixed")
    r = Runner(_index(c), c)
    base = r.snap()[0]
    r.arm()
    new_doc = b"abca" + c.tok[63] + b"dd" + c.tok[2] + b"cab" + c.tok[64] + b"a"
    r.t.add(777_777, new_doc)
    r.t.build()
    c2 = c.with_doc(777_777, new_doc)
    r.c = c2
    r.parts = [(r.t, c2, r.parts[0][2])]
    r.parts[0][2].rebuilt()
    assert r.snap()[0]["batches"] == base["batches"] + 2          # (reset + arm: the build has not touched the counters)
    p = r.batch([c.tok[63], c.tok[2], c.tok[1]] + c.pool()[:30], what="f after build")   # 64, 3 and 1 hits now
    assert (p["spec"], p["wave"]) == (0, 1) and c2.hits(c.tok[63]) == 64
    p = r.batch([c.tok[1], c.tok[64], c.tok[63]], what="f 65 hits now")
    assert (p["spec"], p["spills"], p["sort"]) == (1, 1, 1) and c2.hits(c.tok[64]) == 65
    # save, then load into a second handle that is armed for another corpus
    path = str(tmp_path / "paths.cdb")
    r.t.save(path)
    cs = corpus_of("small")
    r2 = Runner(_index(cs), cs)
    r2.arm()
    before = r2.snap()[0]
    r2.t.load(path)
    r2.c = c2
    r2.parts = [(r2.t, c2, r2.parts[0][2])]
    r2.parts[0][2].rebuilt()
    assert r2.snap()[0] == before
    p = r2.batch([c.tok[63], c.tok[2], c.tok[1]] + c.pool()[:30], what="f after load")
    assert (p["spec"], p["wave"]) == (0, 1)
    assert r2.batch(fits_batch(c2, 40, 8), what="f load next")["spec"] == 1
    r2.t.close()
    r.t.close()
    # proof repair: one swapped pair of lowercase suffixes (the keywords below are uppercase: right before and after the repair)
    g = capi.GpuStringIndex()
    g.add_bulk(c.ids, c.blob, c.ds)
    g.set_option("debug_damage_after_build", len(c.text) * 3 // 4)
    g.build()
    r3 = Runner(g, c)
    up = [c.tok[h] for h in (1, 2, 63, 64)] * 4
    assert r3.batch(up, what="f arm before repair")["wave"] == 1
    repaired_already = g.proof_wait(0) == 3
    assert g.proof_wait(60_000) == 3 and g.stat("self_check_fallbacks") == 1
    if repaired_already:      # the repair may have run before the arming batch got the handle: then the order is unknown — start over
        r3.reset()            # from a known state (the repair is still behind us, the results below are still checked)
    else:
        r3.parts[0][2].rebuilt()
    p = r3.batch(up + c.pool()[:20], what="f after repair")
    assert (p["spec"], p["wave"]) == (0, 1)
    assert r3.batch(up, what="f repair next")["spec"] == 1
    g.close()


@gpu
@pytest.mark.parametrize("kind", ["mixed", "wide", "high", "small"])
def test_g_pattern_counts_across_the_search_and_scan_switches(runners, kind):
    r = runners(kind)
    c = r.c
    r.reset()
    for npat in (1, 3, 4, 5, 4096, 4097):
        rng = np.random.default_rng(npat)
        light = [k for k in c.pool() if c.hits(k) <= 3] + [c.tok[1], c.tok[2]] + list(MISSES)
        kws = [light[int(i)] for i in rng.integers(len(light), size=npat)]
        for j in range(0, npat, 97):                              # some lists at 64 hits, the first and (4097) the last among them
            kws[j] = c.tok[64]
        kws[-1] = c.tok[64]
        for device in (False, True):
            r.batch(kws, device=device, what=f"g {npat}")


@gpu
@pytest.mark.parametrize("opt", [("wave_rows", 0, 1), ("query_hit_budget", 1, 1 << 31), ("query_hit_budget", 700, 1 << 31),
                                 ("fast_search", 0, 1), ("search_lanes", 8, 0)])
@pytest.mark.parametrize("kind", ["mixed", "wide", "high", "small"])
def test_h_ab_forms(runners, kind, opt):
    r = runners(kind)
    c = r.c
    name, value, default = opt
    r.reset()
    r.set_option(name, value)
    try:
        r.batch(fits_batch(c, 120, 9), what="h wave class")
        r.batch(fits_batch(c, 120, 10), what="h wave class again")
        kws = fits_batch(c, 120, 11)
        p = r.batch(kws[:60] + [c.tok[65]] + kws[60:] + [c.tok[max(c.tok)]], what="h long lists")
        assert p["sort"] == 1
        if (name, value) == ("query_hit_budget", 1):
            assert p["chunks"] > 1
        r.batch(kws + [c.tok[65]], offsets=True, what="h offsets")
        r.batch(exact_total(c, 4097), what="h 4097")
        r.batch(exact_total(c, 4097), what="h 4097 again")
    finally:
        r.set_option(name, default)


@gpu
@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("kind", ["one_doc", "per_doc", "mixed", "wide", "high", "high_plain", "small"])
def test_i_lone_keywords(runners, kind, resident):
    r = runners(kind)
    c = r.c
    kws = [MISSES[0], MISSES[2]] + [c.tok[h] for h in (1, 63, 64, 65, 4095, 4096, 4097) if h in c.tok] + [b"AAA"]
    r.t.set_option("resident_query", resident)
    try:
        r.reset()
        for kw in kws:
            r.lone(kw, "not armed")
        for kw in kws:                                            # (a list over 4096 hits goes through the batch path and disarms)
            r.arm()
            p = r.lone(kw, "armed")
            if c.hits(kw) > 4096:
                assert (p["spec"], p["spills"], p["sort"]) == (1, 1, 1)
            else:
                assert r.batch(fits_batch(c, 30, 12), what="i still armed")["spec"] == 1
    finally:
        r.t.set_option("resident_query", 2)


@gpu
@pytest.mark.parametrize("kind", ["mixed", "per_doc"])
def test_j_three_shards_keep_their_own_state(kind):
    from coffeedb_amd import capi
    c = corpus_of(kind)
    sh = capi.GpuShards([0, 0, 0])
    sh.set_option("use_all_devices", 1)
    sh.add_bulk(c.ids, c.blob, c.ds)
    sh.build()
    assert sh.count == 3
    bounds = [sh.first_doc(i) for i in range(4)]
    assert bounds[0] == 0 and bounds[3] == len(c.docs)
    parts = [(sh.shard(i), Corpus(c.docs[bounds[i]:bounds[i + 1]], c.ids[bounds[i]:bounds[i + 1]], c.tok, f"{kind}/{i}"), Model())
             for i in range(3)]
    r = Runner(sh, c, parts)
    seq_a(r)
    for where, long_h in (("middle", 65), ("first", 65), ("last", 64)):
        seq_b(r, where, long_h)
    seq_c(r)
    sh.close()


@gpu
def test_k_two_threads_one_handle(runners):
    r = runners("mixed")
    c = r.c
    r.reset()
    before = r.snap()[0]
    errors = []

    def client(t):
        try:
            for i in range(20):
                kws = fits_batch(c, 40, 100 * t + i)
                if t:
                    kws.insert(i % 41, c.tok[65])
                want = c.expect(kws)
                got = r.t.query_batch(*_pack(kws))
                if not (got[3] == want[3] and all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3]))):
                    errors.append((t, i))
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(repr(e))
    threads = [threading.Thread(target=client, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[:3]
    after = r.snap()[0]
    d = {k: after[k] - before[k] for k in STATS}
    assert d["batches"] == 40 and d["spec"] + d["wave"] + d["sort"] + d["empty"] - d["spills"] == 40, d
    assert d["sort"] == 20 and d["empty"] == 0 and d["chunks"] == 20, d


@gpu
@pytest.mark.parametrize("seed", range(FUZZ_N))
def test_fuzz_sequences(runners, seed):
    r = runners("mixed")
    budget, steps = fuzz_plan(r.c, seed)
    r.reset()
    r.set_option("query_hit_budget", budget)
    try:
        for kind, kws, pred in steps:
            if kind == "rebuild":
                r.t.build()
                r.parts[0][2].rebuilt()
                continue
            p = r.batch(kws, offsets=kind == "offsets", what=f"fuzz {seed} {kind}")
            assert {k: p[k] for k in STATS} == {k: pred[k] for k in STATS}   # (the plan's model and the runner's walked the same path)
    finally:
        r.set_option("query_hit_budget", 1 << 31)
