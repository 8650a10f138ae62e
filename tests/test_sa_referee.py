"""The referee of tests/test_gpu_verify.py, pinned on the CPU: it finds nothing on the arrays of the independent model
(tests/ref_model.py), agrees with the oracle's inversion count on damaged ones, and every corpus really reaches the edge
it was made for — so a corpus cannot silently stop covering it."""
import numpy as np
import pytest

from tests import sa_referee as R
from tests.ref_model import RefModel


def _model(docs):
    m = RefModel(range(len(docs)), docs)
    blob, ds = R.pack_docs(docs)
    return m, blob, ds


def _judge(m, blob, ds, sa=None, **kw):
    return R.judge(m.sa if sa is None else sa, blob, ds, m.bits, m.mask, **kw)


def _all_zero(v, mixed=False):
    assert v.tie_violations == 0 and v.ref_violations == 0 and v.entry_sum == v.expected_entry_sum
    assert v.full_check_bad(plain=not mixed) == 0
    if not mixed:
        assert v.inversions == 0 and v.mixed_pairs == 0 and v.node_pairs == 0


@pytest.fixture(scope="module")
def heads():
    docs = R.heads_docs()
    return (docs,) + _model(docs)


def test_heads_reaches_every_head_length_in_every_kind(heads):
    docs, m, blob, ds = heads
    assert m.width == 4 and 4000 < m.size < 4700 and m.size > 4 * 256
    assert 0 < len(docs[-1]) < 16                            # a 16-byte window past the end of the text
    assert 0x00 in blob and set(np.unique(blob)) == {0x00, 0x01, 0x61, 0x62}
    v = _judge(m, blob, ds, walk_cap=4096)
    _all_zero(v)
    for kind, lengths in ((R.SAME, range(0, 34)), (R.PREFIX, range(1, 34)), (R.TIE, range(1, 34))):
        have = set(v.lcp[v.kind == kind].tolist())
        assert set(lengths) <= have, (kind, sorted(set(lengths) - have))
    assert np.count_nonzero(v.short < 8) and np.count_nonzero((v.short >= 8) & (v.short < 16))


def test_heads8_has_eight_byte_entries():
    docs = R.heads8_docs()
    m, blob, ds = _model(docs)
    assert m.width == 8 and m.bits == 17 and max(map(len, docs)) == 32769
    _all_zero(_judge(m, blob, ds, walk_cap=4096))


@pytest.mark.parametrize("extra", [0, 1])
def test_mixed_sits_on_the_bucket_size_threshold(extra):
    docs = R.mixed_docs(extra)
    m, blob, ds = _model(docs)
    n = m.size
    assert m.width == 4 and m.chuck == 4096 and 10_000 < n < 10_800
    v = _judge(m, blob, ds, walk_cap=4096)
    _all_zero(v, mixed=True)
    assert v.inversions > 0                                  # the reference's order is not sorted where mixed nodes exist
    # the pairs of the plain corpus (root, 'q', 'r': 3 mixed, 1 + extra of them in radix nodes) and the one of the 0x80 bucket
    assert (v.mixed_pairs, v.node_pairs) == (4, 1 + extra)
    mixed = np.flatnonzero(v.kind == R.MIXED)
    q = [j for j in mixed if v.lcp[j] == 1 and R.suffix_bytes(m.sa, blob, ds, m.bits, m.mask, v.at[j])[:1] == b"q"]
    assert len(q) == 1 and v.run[q[0]] == min(4096 + extra, 4097) and bool(v.node[q[0]]) == bool(extra)
    assert bool(v.high_first[q[0]]) == bool(extra)            # ASCII first in the leaf, bytes >= 0x80 first in the node
    first, last = R.mixed_edge_pairs(v)
    assert first is not None and last is not None and first != last
    # a suffix that is a prefix of its right neighbour, whose next byte is >= 0x80: a prefix, not a mixed pair
    suffix = lambda i: R.suffix_bytes(m.sa, blob, ds, m.bits, m.mask, i)
    assert any(suffix(i)[len(suffix(i - 1))] >= 0x80 for i in v.at[(v.kind == R.PREFIX) & ~v.bad_prefix])


def test_mixed_edge_buckets_touch_both_ends_of_the_array():
    docs = R.mixed_docs(1)
    m, blob, ds = _model(docs)
    v = _judge(m, blob, ds)
    first, last = R.mixed_edge_pairs(v)
    suffix = lambda i: R.suffix_bytes(m.sa, blob, ds, m.bits, m.mask, i)
    assert suffix(0)[:1] == suffix(first)[:1] == b"\x80" and suffix(first - 1)[:1] == b"\x80"
    assert suffix(m.size - 1)[:1] == suffix(last)[:1] == b"r" and suffix(last - 1)[:1] == b"r"


def test_long_reaches_the_walk_limit():
    docs, k = R.long_docs()
    assert all(len(d) >= 5000 for d in docs[:3]) and docs[3] == docs[0][k:k + 4096] and docs[0][k + 4096] != 0x61
    m, blob, ds = _model(docs)
    v = _judge(m, blob, ds, walk_cap=4096)
    _all_zero(v)
    p = R.long_pairs(v)
    assert set(p) == {"lcp4095", "lcp4096_longer", "lcp4096_ends"}
    sa = np.asarray(m.sa, dtype=np.uint32)
    base = R.judge(sa, blob, ds, m.bits, m.mask, walk_cap=4096)
    assert base.full_check_bad(plain=True) == 0 and base.inversions == 0
    for name, judged in (("lcp4095", 1), ("lcp4096_longer", 0), ("lcp4096_ends", 1)):
        i = p[name]
        w = R.judge(R.swap_pairs(sa, [i - 1]), blob, ds, m.bits, m.mask, walk_cap=4096)
        j = int(np.flatnonzero(w.at == i)[0])                # the swapped pair itself ...
        assert w.descend[j] or w.bad_prefix[j]
        assert (w.inversions, w.tie_violations) == (1, 0)     # ... is the only one out of order
        assert bool(w.trusted[j]) == (not judged), name
        assert w.full_check_bad(plain=True) == judged, name
        assert R.judge(R.swap_pairs(sa, [i - 1]), blob, ds, m.bits, m.mask).full_check_bad(plain=True) == 1


def test_seam_corpus_spans_the_sweeps_wraps_in_four_byte_entries():
    blob, ds = R.seam_corpus()
    n, nd = int(ds[-1]), len(ds) - 1
    assert n == len(blob) == (1 << 24) + (1 << 16) and np.all(np.diff(ds.astype(np.int64)) >= 1)
    longest = int(np.diff(ds.astype(np.int64)).max())
    assert nd.bit_length() + longest.bit_length() <= 32        # document bits + offset bits: 4-byte entries
    assert blob.min() >= 0x61 and blob.max() <= 0x6A


def test_referee_counts_the_oracles_inversions(heads):
    from oracle import OracleIndex
    docs, m, blob, ds = heads
    o = OracleIndex()
    o.add_bulk(np.arange(len(docs), dtype=np.int64), blob, ds)
    o.build(1)
    o.canonicalize()
    assert o.bits == m.bits and o.mask == m.mask and np.array_equal(o.sa(), np.asarray(m.sa, dtype=np.uint32))
    n = m.size
    damaged = R.swap_pairs(o.sa(), [0, 63, 64, 255, 256, 1000, 2001, n // 2, n - 2])
    o.sa_view()[:] = damaged
    v = R.judge(damaged, blob, ds, m.bits, m.mask)
    assert v.inversions == o.inversions() > 0
    assert v.entry_sum == v.expected_entry_sum
    for r in range(3):
        damaged = R.swap_pairs(np.asarray(m.sa, dtype=np.uint32), R.third(n, r))
        o.sa_view()[:] = damaged
        v = R.judge(damaged, blob, ds, m.bits, m.mask)
        assert v.inversions == o.inversions() > 1000 and v.tie_violations > 200


def test_referee_judges_a_mixed_pair_by_the_run_around_it():
    """hand-made: 3 of 6 suffixes share 'q'; chuck = 6: all leaves, chuck = 3: the root is a node, chuck = 2: 'q' as well"""
    docs = [b"qA", b"q\xC3", b"qB"]
    blob, ds = R.pack_docs(docs)
    bits, mask = 2, 3
    e = lambda d, o: (o << bits) | d
    leaf = np.array([e(0, 1), e(2, 1), e(0, 0), e(2, 0), e(1, 0), e(1, 1)], dtype=np.uint32)   # A B qA qB qC3 C3: sorted
    v = R.judge(leaf, blob, ds, bits, mask, chuck=6)
    assert (v.inversions, v.ref_violations, v.mixed_pairs, v.node_pairs) == (0, 0, 2, 0)
    v = R.judge(leaf, blob, ds, bits, mask, chuck=2)           # 'q' (3 > 2) and the root (6 > 2) are nodes now: high bytes first
    assert (v.inversions, v.ref_violations, v.mixed_pairs, v.node_pairs) == (0, 2, 2, 2)
    assert v.full_check_bad(plain=True) == 0 and v.full_check_bad(plain=False) == 2
    assert v.full_check_bad(plain=False, judge_mixed=False) == 0
    node = np.array([e(1, 1), e(0, 1), e(2, 1), e(1, 0), e(0, 0), e(2, 0)], dtype=np.uint32)   # C3 A B | qC3 qA qB
    v = R.judge(node, blob, ds, bits, mask, chuck=2)
    assert (v.inversions, v.ref_violations, v.mixed_pairs, v.node_pairs) == (2, 0, 2, 2)
    assert v.entry_sum == v.expected_entry_sum
    v = R.judge(node, blob, ds, bits, mask, chuck=3)           # only the root is a node: 'q' should have been sorted
    assert (v.ref_violations, v.mixed_pairs, v.node_pairs) == (1, 2, 1)
