"""cdb_append / cdb_debug_verify_keys without a GPU: both symbols are declared, exported and listed by the binding, the argument
checks answer before any device is touched, and the argument the merge rests on holds on the CPU restatement of the reference
(tests/ref_model.py): the suffix array over "old documents, then new documents" is the stable merge of the old documents' array
and the new documents' array, ties old first, after both are re-encoded in the joint layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from coffeedb_amd import capi
from tests.ref_model import RefModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_append", "cdb_debug_verify_keys")
CDB_E_INVALID = 1


@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.load_library()


def test_symbols_declared_exported_and_listed(lib):
    header = open(os.path.join(ROOT, "include", "coffeedb_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} is not declared in include/coffeedb_gpu.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.EXPORTS
    assert callable(capi.GpuStringIndex.append) and callable(capi.GpuStringIndex.verify_keys)


def test_null_arguments_are_invalid_without_a_device(lib):
    fake = C.c_void_p(8)   # never dereferenced: the checks below fail before the handle is looked at
    n = C.c_uint64(0)
    ids = np.array([1, 2], dtype=np.int64)
    blob = np.frombuffer(b"abcd", dtype=np.uint8)
    ds = np.array([0, 2, 4], dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.cdb_append(None, p(ids), p(blob), p(ds), 2, C.byref(n)) == CDB_E_INVALID      # NULL handle
    assert lib.cdb_append(None, None, None, None, 0, None) == CDB_E_INVALID
    assert lib.cdb_append(fake, None, p(blob), p(ds), 2, C.byref(n)) == CDB_E_INVALID        # documents announced, no ids
    assert lib.cdb_append(fake, p(ids), None, p(ds), 2, C.byref(n)) == CDB_E_INVALID         # ... no blob
    assert lib.cdb_append(fake, p(ids), p(blob), None, 2, C.byref(n)) == CDB_E_INVALID       # ... no doc_start
    out = (C.c_uint64 * 2)()
    assert lib.cdb_debug_verify_keys(None, out) == CDB_E_INVALID
    assert lib.cdb_debug_verify_keys(fake, None) == CDB_E_INVALID


# ---- the merge argument ---------------------------------------------------------------------------------------------------
def _suffix(model, e):
    return model.docs[e & model.mask][e >> model.bits:]


def merged_array(old, new, joint):
    """stable two-way merge of the two models' arrays, ties old first, every entry re-encoded as (off << joint.bits) | doc with
    the new documents numbered from len(old.docs)"""
    a = [(_suffix(old, e), ((e >> old.bits) << joint.bits) | (e & old.mask)) for e in old.sa]
    b = [(_suffix(new, e), ((e >> new.bits) << joint.bits) | ((e & new.mask) + len(old.docs))) for e in new.sa]
    out, i, j = [], 0, 0
    while i < len(a) or j < len(b):
        if j == len(b) or (i < len(a) and a[i][0] <= b[j][0]):   # equal counts as "<=": the old entry goes first
            out.append(a[i][1])
            i += 1
        else:
            out.append(b[j][1])
            j += 1
    return out


def _corpus(seed, ndocs, alphabet, maxlen):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, alphabet, size=int(rng.integers(0, maxlen + 1)), dtype=np.uint8) + ord("a")) for _ in range(ndocs)]


CASES = [
    ([b"abracadabra", b"", b"banana", b"banana", b"abra", b"cadabra banana"], [b"banana", b"abra", b"abracadabra!", b"ban", b""]),
    (_corpus(1, 40, 2, 12), _corpus(2, 25, 2, 12)),                       # two letters: many twins and prefixes across the halves
    (_corpus(3, 30, 3, 20), _corpus(3, 30, 3, 20)),                       # the new documents are copies of the old ones
    (_corpus(4, 5, 4, 9), _corpus(5, 70, 4, 40)),                         # m > n; document and offset fields both grow
    ([b"\x90\xff", b"zz\x80", b"a"], [b"\xff", b"a\x90", b"\x90\xff\x01"]),  # bytes >= 0x80 below the reference's bucket size: unsigned order
]


@pytest.mark.parametrize("old_docs,new_docs", CASES)
def test_fresh_array_is_the_stable_merge(old_docs, new_docs):
    old = RefModel(range(len(old_docs)), old_docs)
    new = RefModel(range(len(new_docs)), new_docs)
    joint = RefModel(range(len(old_docs) + len(new_docs)), list(old_docs) + list(new_docs))
    assert joint.size <= joint.chuck   # (one sorted leaf: the globally sorted case the merge is valid for)
    assert merged_array(old, new, joint) == joint.sa
