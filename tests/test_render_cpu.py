"""cdb_render_rows without a GPU: the three new C-ABI symbols (declared, exported, listed), the layout of cdb_rendered as the
binding sees it, and the argument checks that answer before any device is touched."""
import ctypes as C
import os
import re

import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_render_rows", "cdb_shards_render_rows", "cdb_rendered_free")
FIELDS = ["nrows", "missing", "nspans", "text_bytes", "found", "text_ptr", "text_blob", "span_ptr", "begin", "end"]
CDB_E_INVALID = 1


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
    assert re.search(r"#define\s+CDB_RENDER_TEXT\s+1\b", header) and re.search(r"#define\s+CDB_RENDER_SPANS\s+2\b", header)
    assert (capi.RENDER_TEXT, capi.RENDER_SPANS) == (1, 2)


def test_struct_layout_is_as_declared():
    header = open(os.path.join(ROOT, "include", "coffeedb_gpu.h")).read()
    body = header.split("typedef struct cdb_rendered {")[1].split("} cdb_rendered;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert declared == FIELDS
    assert [f[0] for f in capi.CdbRendered._fields_] == FIELDS
    assert C.sizeof(capi.CdbRendered) == 80
    assert [getattr(capi.CdbRendered, f).offset for f in FIELDS] == list(range(0, 80, 8))


def test_null_arguments_are_invalid_without_a_device(lib):
    out = capi.CdbRendered()
    ids = (C.c_int64 * 2)(1, 2)
    offs = (C.c_uint64 * 2)(0, 1)
    fake = C.c_void_p(8)   # never dereferenced: the checks below fail before the handle is looked at
    for fn in (lib.cdb_render_rows, lib.cdb_shards_render_rows):
        assert fn(None, ids, 2, b"a", offs, 1, None, 0, None, 0, 3, C.byref(out)) == CDB_E_INVALID      # NULL handle
        assert fn(fake, ids, 2, b"a", offs, 1, None, 0, None, 0, 3, None) == CDB_E_INVALID              # NULL out
        assert fn(fake, None, 2, b"a", offs, 1, None, 0, None, 0, 3, C.byref(out)) == CDB_E_INVALID     # rows without ids
        assert fn(fake, ids, 2, b"a", None, 1, None, 0, None, 0, 3, C.byref(out)) == CDB_E_INVALID      # keywords without offsets
        assert fn(fake, ids, 2, b"a", offs, 1, None, 3, None, 0, 3, C.byref(out)) == CDB_E_INVALID      # left_len without left


def test_free_of_null_and_of_a_zero_struct_is_harmless(lib):
    lib.cdb_rendered_free(None)
    zero = capi.CdbRendered()
    lib.cdb_rendered_free(C.byref(zero))
    assert zero.nrows == 0 and not zero.found and not zero.text_blob
