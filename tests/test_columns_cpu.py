"""Numeric / bool columns (cdb_column_*): the parts that need no GPU — the C ABI is declared and exported, every entry
point refuses NULL arguments, and without a gfx950 device there is no CPU fallback."""
import ctypes as C
import os
import re

import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cdb_column_create", "cdb_column_destroy", "cdb_column_last_error", "cdb_column_add_bulk", "cdb_column_build",
       "cdb_column_query", "cdb_column_query_any", "cdb_query_and_columns", "cdb_column_get_stat"]


@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.load_library()


def test_column_symbols_declared_and_exported(lib):
    src = open(os.path.join(ROOT, "include", "coffeedb_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cdb_[a-z_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
    assert "cdb_column_key" in src and "typedef struct cdb_column cdb_column" in src


def test_column_entry_points_refuse_null_arguments(lib):
    INVALID = 1
    ids = (C.c_int64 * 1)(7)
    vals = (C.c_int64 * 1)(3)
    out_ids, n = C.POINTER(C.c_int64)(), C.c_size_t(0)
    out_cnt = C.POINTER(C.c_int64)()
    v = C.c_double(0)
    assert lib.cdb_column_create(None, -1, 1) == INVALID
    h = C.c_void_p()
    assert lib.cdb_column_create(C.byref(h), -1, 7) == INVALID  # no such kind
    assert lib.cdb_column_add_bulk(None, ids, vals, 1) == INVALID
    assert lib.cdb_column_build(None) == INVALID
    assert lib.cdb_column_query(None, b"[1,2]", 5, C.byref(out_ids), C.byref(n)) == INVALID
    off = (C.c_uint64 * 2)(0, 5)
    assert lib.cdb_column_query_any(None, b"[1,2]", off, 1, C.byref(out_ids), C.byref(n)) == INVALID
    assert lib.cdb_column_get_stat(None, b"rows", C.byref(v)) == INVALID
    assert lib.cdb_debug_column_set_option(None, b"profile", 1) == INVALID
    # an AND needs at least one key, and every column key a column
    assert lib.cdb_query_and_columns(None, 0, None, 0, 0, 0, 0, 0, C.byref(out_ids), C.byref(out_cnt), C.byref(n)) == INVALID
    key = capi.CdbColumnKey()
    key.column = None
    assert lib.cdb_query_and_columns(None, 0, C.byref(key), 1, 0, 0, 0, 0, C.byref(out_ids), C.byref(out_cnt), C.byref(n)) == INVALID
    assert lib.cdb_column_last_error(None) == b"null column"
    lib.cdb_column_destroy(None)  # a no-op


def test_column_has_no_cpu_fallback_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    for kind in (0, 1, 2):
        assert lib.cdb_column_create(C.byref(h), -1, kind) == 2  # CDB_E_DEVICE
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        capi.GpuColumn("int64")
