"""Which forms a suffix-array build takes: the build's form statistics and, per kernel name of the profile, its launch and byte
counts, against a recording of an earlier library (tests/golden/build_forms.json).  A correct array does not show that a build
still takes the same path — a flipped form would only be slower — so a change that is meant to leave the build as it is (moving
code between files, say) is held to this recording.  A change that is meant to alter a form records the fixture anew:

    python3 tests/test_gpu_build_forms.py tests/golden/build_forms.json      (twice; fields that differ between two recordings
                                                                              of one library are left out: --merge a.json b.json)
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_forms.json")

STATS = ["key_symbols", "symbol_bits", "digit_bits", "key_layout", "dense_keys", "fused_keygen", "msd_first", "bucketed", "bucket_groups",
         "segmented", "fused_records", "sweep_records", "vl_key_bits", "carried_key_bits", "carried_rounds", "partial_levels", "root_folded",
         "flags_in_last_pass", "pairclass_fused", "gen_prebased", "sort_passes", "sort_passes_skipped", "rounds", "ext_rounds", "dbl_rounds",
         "list_rounds", "group_sorts", "isa_built", "unresolved_after_initial", "unresolved_after_carried", "final_depth", "compat_rotations",
         "compat_depth"]

VL = dict(force_big_path=1, vl_keys=40)


def _W():
    from coffeedb_amd import workloads
    return workloads


@functools.lru_cache(maxsize=None)
def _letters(ndocs):
    return _W().ascii_corpus(ndocs, 256, seed=7, lo=0x61, hi=0x7A)


@functools.lru_cache(maxsize=None)
def _zipf_few_documents():
    # 2^24 bytes, the smallest size at which the key width comes from a sorted sample and the pair count runs beside it on the
    # second stream; 4-byte entries
    return _W().zipf_corpus(16, 1 << 20, seed=3)


@functools.lru_cache(maxsize=None)
def _zipf_many_documents():
    # the same text in 65 536 documents, one of them 8 MiB long: 16 document bits + 24 offset bits, 8-byte entries
    blob = _zipf_few_documents()[0]
    lens = np.full(65536, 128, dtype=np.uint64)
    lens[65536 // 3] += (1 << 24) - 65536 * 128
    return blob, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _zipf_carried():
    # tests/test_gpu_carried_bits.py's shape at 2^20 bytes: 20 000 pairs of 14-byte documents that share their first eight symbols
    # (about 41 code bits: ties the 40-bit key leaves open and the carried bits part) and one long document — 16 document bits +
    # 19 offset bits leave 5 spare bits above a 35-bit entry
    W = _W()
    z = lambda n, seed: W.zipf_corpus(1, n, seed=seed)[0][:n]
    pairs = np.repeat(z(14 * 20000, 31).reshape(20000, 14), 2, axis=0)
    pairs[1::2, 8:] = z(6 * 20000, 32).reshape(20000, 6)
    blob = np.concatenate([pairs.reshape(-1), z((1 << 20) - 40000 * 14, 33)])
    return blob, np.concatenate([np.arange(40001, dtype=np.uint64) * 14, [len(blob)]]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _printable_16m():
    # (Zipf-64 at 2^24 bytes takes 8-symbol keys, wider than the split and MSD-first sorts' 40 bits.  Printable ASCII takes 5 symbols
    #  there, the split sort; with 6 symbols — what it takes from 2^30 bytes on — the keys are dense and the sort is MSD-first)
    return _W().ascii_corpus(16, 1 << 20, seed=5)


@functools.lru_cache(maxsize=None)
def _utf8():
    return _W().utf8_corpus(4096, 256, seed=4)


@functools.lru_cache(maxsize=None)
def _one_symbol():
    return np.full(1 << 14, 0x61, dtype=np.uint8), np.arange(5, dtype=np.uint64) * (1 << 12)


# name -> (corpus, options, what the case is there for: statistics and kernels it must show whatever the recording says)
CASES = {
    "letters_64k": (lambda: _letters(256), {}, {"bucketed": 0}, ()),
    "letters_1m": (lambda: _letters(4096), {}, {"bucketed": 0}, ()),
    "zipf_16m_entries4": (_zipf_few_documents, {}, {"bucketed": 0}, ("sa_tile_paircount", "rs_onesweep_k64_v32_t16384")),
    "zipf_16m_entries8": (_zipf_many_documents, {}, {"bucketed": 0}, ("rs_onesweep_k64_v64_t16384",)),
    "printable_16m_split": (_printable_16m, {}, {"bucketed": 0, "key_layout": 2, "fused_keygen": 1}, ("rs_onesweep_textgen_split_t16384",)),
    "printable_16m_msd_first": (_printable_16m, dict(key_symbols=6), {"bucketed": 0, "dense_keys": 1, "key_layout": 2, "msd_first": 2,
                                                                      "gen_prebased": 1, "flags_in_last_pass": 1}, ("sa_tile_paircount",)),
    "zipf_1m_sweep_segmented_carried": (_zipf_carried, VL, {"bucketed": 1, "sweep_records": 1, "segmented": 1, "vl_key_bits": 40,
                                                              "carried_key_bits": 5, "carried_rounds": 1}, ()),
    "zipf_1m_per_bucket": (_zipf_carried, dict(VL, segmented_sort=0), {"bucketed": 1, "segmented": 0}, ("sa_bucket_records",)),
    "zipf_1m_partition_gather": (_zipf_carried, dict(VL, sweep_records=0, fuse_records=0),
                                 {"bucketed": 1, "sweep_records": 0, "fused_records": 0}, ("sa_gather_plan",)),
    "zipf_1m_three_groups": (_zipf_carried, dict(VL, bucket_group_limit=(1 << 20) * 3 // 8), {"bucketed": 1, "bucket_groups": 3}, ()),
    "utf8_1m_bucketwise": (_utf8, dict(force_big_path=1), {"bucketed": 1, "root_folded": 1}, ("sa_pairclass", "sa_compat_copy")),
    "utf8_1m_direct": (_utf8, {}, {"bucketed": 0, "root_folded": 0}, ("sa_compat_copy",)),
    "one_symbol_doubling": (_one_symbol, dict(force_doubling=1), {"isa_built": 1}, ("sa_isa_init",)),
}


def run_case(name):
    """builds the case's corpus with profile = 1 -> {"stats": {name: value}, "profile": {kernel: [launches, bytes]}, "fallbacks": n}"""
    from coffeedb_amd import capi
    corpus, opts = CASES[name][:2]
    blob, ds = corpus()
    g = capi.GpuStringIndex()
    try:
        g.set_option("profile", 1)
        for k, v in opts.items():
            g.set_option(k, v)
        g.add_bulk(np.arange(len(ds) - 1, dtype=np.int64) + 1, blob, ds)
        g.build()
        return {"stats": {s: g.stat(s) for s in STATS},
                "profile": {k: [v["launches"], v["bytes"]] for k, v in sorted(g.profile().items())},
                "fallbacks": g.stat("self_check_fallbacks") + g.stat("group_fallbacks")}
    finally:
        g.close()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, rec in recorded.items():
        assert rec["fallbacks"] == 0 and rec["profile"], name
        for stat, want in CASES[name][2].items():
            assert rec["stats"][stat] == want, (name, stat, rec["stats"][stat])
        assert set(CASES[name][3]) <= set(rec["profile"]), (name, sorted(rec["profile"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_takes_the_recorded_forms(recorded, name):
    got, rec = run_case(name), recorded[name]
    print(name, json.dumps(got))
    assert got["fallbacks"] == 0
    for stat, want in CASES[name][2].items():
        assert got["stats"][stat] == want, (stat, got["stats"][stat], want)
    differing = {s: (got["stats"][s], v) for s, v in rec["stats"].items() if got["stats"][s] != v}
    assert not differing, differing
    assert set(got["profile"]) == set(rec["profile"]), set(got["profile"]) ^ set(rec["profile"])
    # [launches, bytes] per kernel name (a count the fixture holds as null differed between two recordings of one library)
    differing = {k: (got["profile"][k], v) for k, v in rec["profile"].items()
                 if any(w is not None and h != w for h, w in zip(got["profile"][k], v))}
    assert not differing, differing


def merge(a, b):
    """two recordings of one library -> the fixture: a statistic or a count that differs between them is left out (null for a count)"""
    out, left_out = {}, []
    for name in a:
        ra, rb = a[name], b[name]
        assert set(ra["profile"]) == set(rb["profile"]), name
        stats = {s: v for s, v in ra["stats"].items() if rb["stats"][s] == v}
        left_out += [f"{name}: {s}" for s in ra["stats"] if s not in stats]
        prof = {}
        for k, v in ra["profile"].items():
            prof[k] = [x if x == y else None for x, y in zip(v, rb["profile"][k])]
            left_out += [f"{name}: {k}[{i}]" for i, x in enumerate(prof[k]) if x is None]
        out[name] = {"stats": stats, "profile": prof, "fallbacks": max(ra["fallbacks"], rb["fallbacks"])}
    return out, left_out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--merge":
        with open(sys.argv[2]) as fa, open(sys.argv[3]) as fb:
            fixture, left_out = merge(json.load(fa), json.load(fb))
        print("left out:", left_out)
        with open(sys.argv[4], "w") as f:
            f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(fixture[k], sort_keys=True) for k in sorted(fixture)) + "\n}\n")
    else:
        from coffeedb_amd import capi
        capi.load_library()
        with open(sys.argv[1], "w") as f:
            json.dump({name: run_case(name) for name in sorted(CASES)}, f, indent=1, sort_keys=True)
            f.write("\n")
