"""cdb_remove / cdb_column_remove without a GPU: both symbols are declared, exported and listed by the binding, and the
argument checks answer before any device is touched."""
import ctypes as C
import os
import re

import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_remove", "cdb_column_remove")
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
    assert callable(capi.GpuStringIndex.remove) and callable(capi.GpuColumn.remove)


def test_null_arguments_are_invalid_without_a_device(lib):
    fake = C.c_void_p(8)   # never dereferenced: the check below fails before the handle is looked at
    n = C.c_uint64(0)
    for fn in (lib.cdb_remove, lib.cdb_column_remove):
        assert fn(None, None, 0, C.byref(n), C.byref(n)) == CDB_E_INVALID      # NULL handle
        assert fn(fake, None, 2, C.byref(n), C.byref(n)) == CDB_E_INVALID      # ids announced, none given
