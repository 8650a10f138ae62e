"""cdb_shards_remove / cdb_shards_append / cdb_shards_cluster without a GPU: the three symbols are declared, exported and listed
by the binding, and the argument checks answer before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_shards_remove", "cdb_shards_append", "cdb_shards_cluster")
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
    for method in ("remove", "append", "cluster"):
        assert callable(getattr(capi.GpuShards, method, None)), f"GpuShards.{method} is missing"


def test_header_no_longer_excludes_sharded_columns():
    header = open(os.path.join(ROOT, "include", "coffeedb_gpu.h")).read()
    assert "Not available on cdb_shards" not in header


def test_null_arguments_are_invalid_without_a_device(lib):
    fake = C.c_void_p(8)   # never dereferenced: the checks below fail before the handle is looked at
    n, m = C.c_uint64(0), C.c_uint64(0)
    ids = np.array([1, 2], dtype=np.int64)
    blob = np.frombuffer(b"abcd", dtype=np.uint8)
    ds = np.array([0, 2, 4], dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.cdb_shards_remove(None, p(ids), 2, C.byref(n), C.byref(m)) == CDB_E_INVALID      # NULL handle
    assert lib.cdb_shards_remove(None, None, 0, None, None) == CDB_E_INVALID
    assert lib.cdb_shards_remove(fake, None, 2, C.byref(n), C.byref(m)) == CDB_E_INVALID        # ids announced, none given
    assert lib.cdb_shards_append(None, p(ids), p(blob), p(ds), 2, C.byref(n)) == CDB_E_INVALID  # NULL handle
    assert lib.cdb_shards_append(None, None, None, None, 0, None) == CDB_E_INVALID
    assert lib.cdb_shards_append(fake, None, p(blob), p(ds), 2, C.byref(n)) == CDB_E_INVALID    # documents announced, no ids
    assert lib.cdb_shards_append(fake, p(ids), None, p(ds), 2, C.byref(n)) == CDB_E_INVALID     # ... no blob
    assert lib.cdb_shards_append(fake, p(ids), p(blob), None, 2, C.byref(n)) == CDB_E_INVALID   # ... no doc_start
    out = capi.CdbClusters()
    assert lib.cdb_shards_cluster(None, p(ids), 2, 1, C.byref(out)) == CDB_E_INVALID            # NULL handle
    assert lib.cdb_shards_cluster(fake, p(ids), 2, 1, None) == CDB_E_INVALID                    # no result
    assert lib.cdb_shards_cluster(fake, None, 2, 1, C.byref(out)) == CDB_E_INVALID              # rows announced, none given
