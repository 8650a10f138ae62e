"""The verifiers of verify.hip as judges: cdb_debug_verify, cdb_debug_verify_reference, the full sweep behind
self_check = 2 and the order proof (sa_full_check_kernel), against the CPU referee of tests/sa_referee.py.

Every correctness claim of the full-size tests and every "proved" build ends in these kernels, so each is given arrays
damaged in EVERY adjacent pair once (three loads: the pairs k = r mod 3), single damages at the first and last pair and at
wavefront and workgroup boundaries, text whose suffixes first differ, end or tie at every length around the 16-byte head
the sweep compares first, real 0x00 bytes, a reference-order bucket of exactly chuck_size and chuck_size + 1 suffixes,
common prefixes at the 4096-byte walk limit, and the grid-stride and slice seams of the sweep.  Every comparison is an
exact integer equality with the referee's count.

Damage reaches a handle through a saved file whose entries (its tail) are patched and which is loaded with
self_check = 1, so no proof repairs it; or through the hook debug_damage_after_build, where the proof is the subject."""
import time

import numpy as np
import pytest

from tests import sa_referee as R
from tests.ref_model import RefModel

pytestmark = pytest.mark.gpu

CASES = {  # name -> (documents, options of the handle, entry width, stat sa_packed)
    "heads": (lambda: R.heads_docs(), {}, 4, 0),
    "heads8": (lambda: R.heads8_docs(), {}, 8, 1),
    "heads8-plain": (lambda: R.heads8_docs(), {"pack_sa": 0}, 8, 0),
    "mixed0": (lambda: R.mixed_docs(0), {}, 4, 0),
    "mixed1": (lambda: R.mixed_docs(1), {}, 4, 0),
    "long": (lambda: R.long_docs()[0], {}, 4, 0),
}


class Case:
    """one corpus built on the GPU in one storage form: the true array, its file and the referee's view of it"""

    def __init__(self, name, tmp):
        from coffeedb_amd import capi
        make, self.opts, width, packed = CASES[name]
        self.name, self.mixed = name, name.startswith("mixed")
        docs = make()
        self.blob, self.ds = R.pack_docs(docs)
        m = RefModel(range(len(docs)), docs)
        self.bits, self.mask, self.n = m.bits, m.mask, m.size
        self.dtype = np.uint32 if width == 4 else np.uint64
        self.sa = np.asarray(m.sa, dtype=self.dtype)
        assert capi.layout_rule(len(docs), max(map(len, docs)))[:3] == (self.bits, self.mask, width)
        g = self.handle()
        g.add_bulk(np.arange(len(docs), dtype=np.int64), self.blob, self.ds)
        g.build()
        assert g.sa_width == width and g.stat("sa_packed") == packed and (g.bits, g.mask, g.size) == (self.bits, self.mask, self.n)
        assert np.array_equal(g.sa(), self.sa)                # the build is the independent model's array
        self.g = g
        self.path = str(tmp / (name + ".cdb"))
        g.save(self.path)
        raw = open(self.path, "rb").read()
        self.head = raw[:len(raw) - self.n * width]           # (the entries are the file's tail)
        assert np.array_equal(np.frombuffer(raw[len(self.head):], dtype=self.dtype), self.sa)
        self.bad_path = str(tmp / (name + ".damaged.cdb"))

    def handle(self, self_check=None):
        from coffeedb_amd import capi
        g = capi.GpuStringIndex()
        if self_check is not None:
            g.set_option("self_check", self_check)
        for k, v in self.opts.items():
            g.set_option(k, v)
        return g

    def judge(self, sa):
        return R.judge(sa, self.blob, self.ds, self.bits, self.mask, walk_cap=4096)

    def load(self, sa, self_check=1):
        """a handle over the file with `sa` as its entries; self_check = 1: nothing behind the load repairs them"""
        with open(self.bad_path, "wb") as f:
            f.write(self.head)
            f.write(np.ascontiguousarray(sa, dtype=self.dtype).tobytes())
        h = self.handle(self_check)
        h.load(self.bad_path)
        assert h.sa_width == self.g.sa_width and h.stat("sa_packed") == self.g.stat("sa_packed")
        return h

    def check(self, h, v, permutation=True):
        """every verifier's count on handle h equals the referee's verdict v"""
        ver, sweep, ref = h.verify(), h.self_check(full=True), h.verify_reference()
        got = {"inversions": ver["inversions"], "tie_violations": ver["tie_violations"], "invalid_entries": ver["invalid_entries"],
               "entry_sum": ver["entry_sum"], "expected_entry_sum": ver["expected_entry_sum"], "full_sweep": sweep,
               "ref_violations": ref["violations"], "ref_mixed_pairs": ref["mixed_pairs"], "ref_node_pairs": ref["radix_node_pairs"],
               "ref_tie_violations": ref["tie_violations"]}
        # the full sweep: unsigned order where the array claims it, else the reference's order with every bucket judged
        bad = v.full_check_bad(plain=not self.mixed)
        if self.mixed:
            assert bad == v.ref_violations + v.tie_violations      # (no suffix here reaches the walk limit)
        want = {"inversions": v.inversions, "tie_violations": v.tie_violations, "invalid_entries": 0, "entry_sum": v.entry_sum,
                "expected_entry_sum": v.expected_entry_sum, "full_sweep": (bad, 0), "ref_violations": v.ref_violations,
                "ref_mixed_pairs": v.mixed_pairs, "ref_node_pairs": v.node_pairs, "ref_tie_violations": v.tie_violations}
        print(self.name, "gpu", got)
        print(self.name, "referee", want)
        assert got == want
        assert (ver["entry_sum"] == ver["expected_entry_sum"]) == permutation


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(name, tmp_path_factory.mktemp(name))
        return built[name]
    yield get
    for c in built.values():
        c.g.close()


@pytest.mark.parametrize("name", list(CASES))
def test_undamaged_array_is_clean_for_every_verifier(case, name):
    c = case(name)
    v = c.judge(c.sa)
    assert v.tie_violations == 0 and v.ref_violations == 0 and v.full_check_bad(plain=not c.mixed) == 0
    assert (v.inversions > 0) == c.mixed                       # the reference's order is not sorted where mixed nodes exist
    c.check(c.g, v)
    assert c.g.self_check() == (0, 0)                          # (the sampled form)
    # the proof behind the build judged every pair, the bucket-size-dependent ones included
    assert c.g.proof_wait(60_000) == 2 and c.g.stat("proof_pairs") == c.n - 1
    assert c.g.stat("proof_bad_pairs") == 0 and c.g.stat("proof_invalid_entries") == 0 and c.g.stat("proof_skipped_pairs") == 0
    assert c.g.stat("proof_mixed_pairs") == v.mixed_pairs and c.g.stat("self_check_fallbacks") == 0


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_every_pair_swapped_once(case, name, r):
    """The pairs (k, k + 1), k = r mod 3, exchanged: over r = 0, 1, 2 every adjacent pair of the true array is damaged once
    (and its neighbours are judged beside a swapped entry).  A single misjudged pair breaks an equality.

    mixed1, r = 2 is the case that found a defect: the swap at the end of the 'q' bucket (4097 suffixes) leaves a foreign
    entry in its last slot and its last member one slot behind it.  ref_bucket_is_node galloped over the foreign entry and
    counted 4098 entries, a radix node, where the contiguous run around the boundary pair holds 4096, a leaf (full sweep
    3461 instead of 3462, verify_reference 33 violations / 4 node pairs instead of 34 / 3).  The gallop is an upper bound;
    a "node" answer is now confirmed entry by entry (block_bucket_is_node)."""
    c = case(name)
    sa = R.swap_pairs(c.sa, R.third(c.n, r))
    v = c.judge(sa)
    assert v.inversions + v.tie_violations > c.n // 5
    h = c.load(sa)
    try:
        c.check(h, v)
    finally:
        h.close()


def _single(c, sa, permutation=True):
    v = c.judge(sa)
    h = c.load(sa)
    try:
        c.check(h, v, permutation)
    finally:
        h.close()
    return v


@pytest.mark.parametrize("k", [0, 63, 64, 255, 256, -2])
def test_one_swap_at_the_ends_and_at_wave_and_workgroup_boundaries(case, k):
    c = case("heads")
    k = k % c.n
    v = _single(c, R.swap_pairs(c.sa, [k]))
    assert v.inversions + v.tie_violations >= 1


def test_one_duplicated_entry(case):
    c = case("heads")
    sa = c.sa.copy()
    sa[100] = sa[107]
    v = _single(c, sa, permutation=False)
    assert v.entry_sum != v.expected_entry_sum and v.inversions + v.tie_violations >= 1


@pytest.mark.parametrize("k", [0, 64, -2])
@pytest.mark.parametrize("name", ["heads8", "heads8-plain"])
def test_one_swap_in_eight_byte_entries(case, name, k):
    c = case(name)
    v = _single(c, R.swap_pairs(c.sa, [k % c.n]))
    assert v.inversions + v.tie_violations >= 1


def _q_pair(c, v):
    """the one adjacent pair at the boundary between bytes >= 0x80 and < 0x80 inside the bucket of 'q'"""
    q = [int(v.at[j]) for j in np.flatnonzero((v.kind == R.MIXED) & (v.lcp == 1))
         if R.suffix_bytes(c.sa, c.blob, c.ds, c.bits, c.mask, int(v.at[j]))[:1] == b"q"]
    assert len(q) == 1
    return q[0]


@pytest.mark.parametrize("which", ["q", "first", "last"])
@pytest.mark.parametrize("extra", [0, 1])
def test_one_swapped_mixed_pair_is_judged_by_its_bucket_size(case, extra, which):
    """The boundary pair of the 'q' bucket — a leaf of 4096 suffixes (ASCII first) or a radix node of 4097 (bytes >= 0x80 first) —
    and the mixed pairs of the buckets that start at entry 0 and end at entry n - 1: swapped, each is a violation."""
    c = case("mixed%d" % extra)
    true = c.judge(c.sa)
    first, last = R.mixed_edge_pairs(true)
    i = {"q": _q_pair(c, true), "first": first, "last": last}[which]
    v = _single(c, R.swap_pairs(c.sa, [i - 1]))
    j = int(np.flatnonzero(v.at == i)[0])
    assert v.kind[j] == R.MIXED and v.node[j] == (which == "q" and extra == 1) and v.high_first[j] != v.node[j]
    assert v.ref_violations >= 1


@pytest.mark.parametrize("pair", ["lcp4095", "lcp4096_longer", "lcp4096_ends"])
def test_the_walk_limit_of_the_full_sweep(case, pair):
    """verify() counts a swapped pair whatever its common prefix; the full sweep judges it unless 4096 bytes agree and
    neither suffix ends there ("taken on trust beyond 4096")."""
    c = case("long")
    i = R.long_pairs(c.judge(c.sa))[pair]
    v = _single(c, R.swap_pairs(c.sa, [i - 1]))
    assert v.inversions == 1 and v.full_check_bad(plain=True) == (0 if pair == "lcp4096_longer" else 1)


@pytest.mark.parametrize("name", ["heads", "mixed1"])
def test_the_proof_counts_what_the_referee_counts_and_repairs(case, name):
    """The same evidence behind a load with the default self_check = 3: the proof finds exactly the referee's pairs, judges
    every pair, and the handle rebuilds itself into the true array."""
    c = case(name)
    if name == "heads":
        sa = R.swap_pairs(c.sa, R.third(c.n, 0))
    else:
        sa = R.swap_pairs(c.sa, [_q_pair(c, c.judge(c.sa)) - 1])
    v = c.judge(sa)
    h = c.load(sa, self_check=None)
    try:
        assert h.proof_wait(60_000) == 3
        print(name, "proof", h.stat("proof_bad_pairs"), h.stat("proof_mixed_pairs"), "referee", v.full_check_bad(plain=not c.mixed), v.mixed_pairs)
        assert h.stat("proof_bad_pairs") == v.full_check_bad(plain=not c.mixed) > 0
        assert h.stat("proof_pairs") == c.n - 1 and h.stat("proof_skipped_pairs") == 0 and h.stat("proof_invalid_entries") == 0
        assert h.stat("proof_mixed_pairs") == v.mixed_pairs
        assert h.stat("self_check_fallbacks") == 1
        assert np.array_equal(h.sa(), c.sa)
    finally:
        h.close()


# ---- the seams of the sweep: its grid-stride wraps (proof 2^14 workgroups = 2^22 entries, self_check 2^16 = 2^24) and the
# proof's slices of 2^24 entries
class Seams:
    def __init__(self):
        from coffeedb_amd import capi
        self.blob, self.ds = R.seam_corpus()
        self.n = int(self.ds[-1])
        g = capi.GpuStringIndex()
        g.add_bulk(np.arange(len(self.ds) - 1, dtype=np.int64), self.blob, self.ds)
        g.build()
        assert g.size == self.n == (1 << 24) + (1 << 16) and g.sa_width == 4
        assert g.proof_wait(60_000) == 2 and g.stat("proof_pairs") == self.n - 1 and g.stat("proof_bad_pairs") == 0
        self.g, self.sa, self.text = g, g.sa(), self.blob.tobytes()

    def referee(self, ks):
        """the referee's verdict over the pairs beside the swaps at ks (one after the other)"""
        sa = self.sa
        touched = sorted({i for k in ks for i in (k, k + 1, k + 2)})
        lo, hi = touched[0] - 1, touched[-1] + 1                 # a window of the array is enough: pure ASCII, no bucket sizes
        win = R.swap_pairs(sa[lo:hi], [k - lo for k in ks])
        return R.judge(win, self.text, self.ds, self.g.bits, self.g.mask, walk_cap=4096, only=[i - lo for i in touched])


@pytest.fixture(scope="module")
def seams():
    s = Seams()
    yield s
    s.g.close()


@pytest.mark.parametrize("k", [(1 << 22) - 1, 1 << 22, (1 << 24) - 1, 1 << 24])
def test_the_proof_sees_a_swap_at_its_grid_stride_wrap_and_slice_seam(seams, k):
    g = seams.g
    v = seams.referee([k])
    assert v.inversions + v.tie_violations >= 1
    fallbacks = g.stat("self_check_fallbacks")
    t0 = time.perf_counter()
    g.set_option("debug_damage_after_build", k)
    g.build()
    assert g.proof_wait(60_000) == 3
    print("seam", k, "proof_bad_pairs", g.stat("proof_bad_pairs"), "referee", v.full_check_bad(plain=True),
          "wall %.2f s" % (time.perf_counter() - t0))
    assert g.stat("proof_bad_pairs") == v.full_check_bad(plain=True)
    assert g.stat("proof_pairs") == seams.n - 1 and g.stat("self_check_fallbacks") == fallbacks + 1
    assert np.array_equal(g.sa(), seams.sa)                    # restored


def test_the_full_sweep_sees_swaps_at_its_grid_stride_wrap(seams, tmp_path):
    from coffeedb_amd import capi
    t0 = time.perf_counter()
    ks = [(1 << 24) - 1, 1 << 24]
    v = seams.referee(ks)
    path = str(tmp_path / "seam.cdb")
    seams.g.save(path)
    lo = ks[0]
    win = R.swap_pairs(seams.sa[lo:lo + 3], [k - lo for k in ks])
    with open(path, "r+b") as f:                               # (the entries are the file's tail)
        f.seek(-(seams.n - lo) * 4, 2)
        f.write(win.astype("<u4").tobytes())
    h = capi.GpuStringIndex()
    h.set_option("self_check", 1)
    h.load(path)
    try:
        got = h.verify()
        sweep = h.self_check(full=True)
        print("seam file", got, sweep, "referee", v.inversions, v.tie_violations, v.full_check_bad(plain=True),
              "wall %.2f s" % (time.perf_counter() - t0))
        assert (got["inversions"], got["tie_violations"], got["invalid_entries"]) == (v.inversions, v.tie_violations, 0)
        assert got["entry_sum"] == got["expected_entry_sum"] and v.inversions >= 1
        assert sweep == (v.full_check_bad(plain=True), 0)
    finally:
        h.close()
