"""cdb_column_append (and the hook cdb_debug_column_arrays) without a GPU: the symbols are declared, exported and listed by the
binding, and the argument checks answer before any device is touched."""
import ctypes as C
import os
import re

import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_column_append", "cdb_debug_column_arrays", "cdb_column_remove")
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
    assert callable(capi.GpuColumn.append) and callable(capi.GpuColumn.remove) and callable(capi.GpuColumn.arrays)


def test_null_arguments_are_invalid_without_a_device(lib):
    fake = C.c_void_p(8)   # never dereferenced: the checks below fail before the handle is looked at
    n = C.c_uint64(0)
    ids = (C.c_int64 * 2)(1, 2)
    assert lib.cdb_column_append(None, None, None, 0, C.byref(n)) == CDB_E_INVALID        # NULL handle
    assert lib.cdb_column_append(fake, None, ids, 2, C.byref(n)) == CDB_E_INVALID         # rows announced, no ids
    assert lib.cdb_column_append(fake, ids, None, 2, C.byref(n)) == CDB_E_INVALID         # ... no values
    assert lib.cdb_debug_column_arrays(None, None, None, None, None) == CDB_E_INVALID


def test_the_makefile_builds_the_new_source():
    mk = open(os.path.join(ROOT, "coffeedb_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bcolumn_maintain\.hip\b", mk, flags=re.M)
