"""Row sets without a GPU: the new C-ABI symbols (declared, exported, listed), their argument checks and the no-device answer, the
reference-side wrapper coffeedb_amd/csrc/shim/rowset.h against the public header, and the numpy referee of the GPU tests against
Python's own sort."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from coffeedb_amd import capi

from . import rowset_referee as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_filter", "cdb_rowset_free", "cdb_rowset_last_error", "cdb_rowset_size", "cdb_rowset_rows", "cdb_rowset_page",
         "cdb_rowset_cluster", "cdb_rowset_cluster_column", "cdb_rowset_get_stat", "cdb_debug_rowset_from_rows",
         "cdb_debug_rowset_set_option", "cdb_debug_rowset_profile_dump")
CDB_E_INVALID, CDB_E_DEVICE = 1, 2


@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.load_library()


def test_symbols_declared_exported_and_listed(lib):
    header = open(os.path.join(ROOT, "include", "coffeedb_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/coffeedb_gpu.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in capi.EXPORTS
        assert not re.search(r"\d", name)   # the ABI test finds symbols with cdb_[a-z_]+


def test_filter_over_no_keys_is_invalid(lib):
    h = C.c_void_p(7)
    assert lib.cdb_filter(None, 0, None, 0, 0, 0, 0, C.byref(h)) == CDB_E_INVALID
    assert not h.value
    assert lib.cdb_filter(None, 0, None, 0, 0, 0, 0, None) == CDB_E_INVALID
    host = capi.CdbKeyQuery()   # host rows alone: no handle to run the merge on
    assert lib.cdb_filter(C.byref(host), 1, None, 0, 1, 1, 5, C.byref(h)) == CDB_E_INVALID
    assert lib.cdb_filter(None, -1, None, 0, 0, 0, 0, C.byref(h)) == CDB_E_INVALID
    with pytest.raises(RuntimeError, match="no string key and no column"):
        capi.filter_rows([])


def test_null_arguments_are_invalid(lib):
    ids, cnt, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_int64)(), C.c_size_t(0)
    v = C.c_double(0)
    out = capi.CdbClusters()
    assert lib.cdb_rowset_rows(None, C.byref(ids), C.byref(cnt), C.byref(n)) == CDB_E_INVALID
    assert lib.cdb_rowset_page(None, 0, 1, C.byref(ids), C.byref(cnt), C.byref(n)) == CDB_E_INVALID
    assert lib.cdb_rowset_cluster(None, None, 1, C.byref(out)) == CDB_E_INVALID
    assert lib.cdb_rowset_cluster_column(None, None, C.byref(out)) == CDB_E_INVALID
    assert lib.cdb_rowset_get_stat(None, b"rows", C.byref(v)) == CDB_E_INVALID
    assert lib.cdb_debug_rowset_set_option(None, b"profile", 1) == CDB_E_INVALID
    assert lib.cdb_rowset_size(None) == 0
    assert lib.cdb_rowset_last_error(None) == b"null row set"
    lib.cdb_rowset_free(None)
    one = (C.c_int64 * 1)(1)
    h = C.c_void_p()
    assert lib.cdb_debug_rowset_from_rows(-1, None, one, 1, C.byref(h)) == CDB_E_INVALID
    assert lib.cdb_debug_rowset_from_rows(-1, one, one, 1, None) == CDB_E_INVALID


def test_no_row_set_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    one = (C.c_int64 * 1)(1)
    h = C.c_void_p()
    assert lib.cdb_debug_rowset_from_rows(-1, one, one, 1, C.byref(h)) == CDB_E_DEVICE and not h.value
    assert lib.cdb_debug_rowset_from_rows(-1, None, None, 0, C.byref(h)) == CDB_E_DEVICE and not h.value
    with pytest.raises(RuntimeError, match="no usable gfx950 device"):
        capi.debug_rowset_from_rows([1, 2], [3, 4])


def test_shim_header_compiles_against_the_public_header():
    shim = os.path.join(ROOT, "coffeedb_amd", "csrc", "shim", "rowset.h")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", shim])


def test_referee_agrees_with_python_sorted():
    rng = np.random.default_rng(20260)
    ids = np.sort(rng.choice(np.arange(-5000, 5000, dtype=np.int64), 700, replace=False))
    counts = rng.integers(-3, 4, 700).astype(np.int64)
    counts[::50] = -(1 << 63)
    counts[7::90] = (1 << 63) - 1
    want = sorted(zip(ids.tolist(), counts.tolist()), key=lambda r: (-r[1], r[0]))
    ri, rc = R.ranking(ids, counts)
    assert list(zip(ri.tolist(), rc.tolist())) == want
    for first, last in ((0, 1), (0, 700), (3, 40), (699, 700), (10, 10), (700, 900), (650, 9999)):
        pi, pc = R.page(ids, counts, first, last)
        assert list(zip(pi.tolist(), pc.tolist())) == want[first:last]
    assert R.differing_bytes(counts) == 8
    assert R.differing_bytes(np.full(9, 5)) == 0
    assert R.differing_bytes(np.array([1, 200])) == 1
    assert R.differing_bytes(np.array([1 << 40, 2 << 40])) == 1
