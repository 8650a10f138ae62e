"""cdb_column_values / cdb_rowset_select / cdb_selected_free without a GPU: the symbols are declared, exported and listed; the three
structs have the layout the C compiler gives them; every argument check answers CDB_E_INVALID before a handle or a device is
touched (the handles given here are dummies that must never be read); shim/select.h compiles against the public header."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "coffeedb_gpu.h")
SHIM = os.path.join(ROOT, "coffeedb_amd", "csrc", "shim")
NEW = ["cdb_column_values", "cdb_rowset_select", "cdb_selected_free"]
INVALID = 1   # CDB_E_INVALID


@pytest.fixture(scope="module")
def lib():
    capi.build_library()
    return capi.load_library()


def test_symbols_declared_exported_listed(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(cdb_[a-z_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/coffeedb_gpu.h"
        assert name in capi.EXPORTS, f"{name} is not listed in capi.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.cdb_rowset_select.argtypes[3]._type_ is capi.CdbSelectField
    assert lib.cdb_rowset_select.argtypes[-1]._type_ is capi.CdbSelected


LAYOUT = {
    "cdb_select_field": (capi.CdbSelectField, ["index", "shards", "column", "kw_blob", "kw_offsets", "nkw"]),
    "cdb_selected_field": (capi.CdbSelectedField, ["kind", "missing", "found", "values", "text_ptr", "text_blob"]),
    "cdb_selected": (capi.CdbSelected, ["nrows", "nfields", "ids", "counts", "fields"]),
}


def test_struct_layout_as_stated():
    """LP64: pointers and uint64_t are 8 bytes and 8-aligned, the int members are padded up to the next one"""
    want = {"cdb_select_field": (48, [0, 8, 16, 24, 32, 40]), "cdb_selected_field": (48, [0, 8, 16, 24, 32, 40]),
            "cdb_selected": (40, [0, 8, 16, 24, 32])}
    for name, (cls, fields) in LAYOUT.items():
        assert [f for f, _ in cls._fields_] == fields
        assert (C.sizeof(cls), [getattr(cls, f).offset for f in fields]) == want[name], name


def test_struct_layout_equals_the_c_compilers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for name, (_, fields) in LAYOUT.items():
        lines.append(f'    printf("{name} %zu", sizeof({name}));')
        lines += [f'    printf(" %zu", offsetof({name}, {f}));' for f in fields]
        lines.append('    printf("\\n");')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])   # (the header is plain C)
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for name, (cls, fields) in LAYOUT.items():
        assert got[name] == [C.sizeof(cls)] + [getattr(cls, f).offset for f in fields], name


def _garbage_out():
    out = capi.CdbSelected()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    return out


def _is_zeroed(out):
    return bytes(C.string_at(C.byref(out), C.sizeof(out))) == bytes(C.sizeof(out))


def test_rowset_select_argument_checks(lib):
    """None of these may read the row set, a field's handle or a device: the handles are addresses of a scratch buffer."""
    scratch = C.create_string_buffer(256)
    rs, h1, h2, h3 = (C.c_void_p(C.addressof(scratch) + 64 * k) for k in range(4))
    offs = np.array([0, 3], dtype=np.uint64)
    blob = np.frombuffer(b"010", dtype=np.uint8)

    def field(index=None, shards=None, column=None, nkw=0, with_offsets=True):
        f = capi.CdbSelectField()
        f.index, f.shards, f.column = index, shards, column
        if nkw:
            f.kw_blob, f.nkw = blob.ctypes.data, nkw
            f.kw_offsets = offs.ctypes.data if with_offsets else None
        return f

    def call(fields, nfields=None, rs_=rs, out="fresh", left=(None, 0), right=(None, 0)):
        arr = (capi.CdbSelectField * max(len(fields), 1))(*fields) if fields is not None else None
        o = _garbage_out() if out == "fresh" else out
        rc = lib.cdb_rowset_select(rs_, 0, 10, arr, len(fields) if nfields is None else nfields, left[0], left[1], right[0], right[1],
                                   C.byref(o) if o is not None else None)
        if o is not None:
            assert _is_zeroed(o), "a failed call leaves *out zeroed"
        return rc

    assert call([], out=None) == INVALID                                        # NULL out
    assert call([], rs_=None) == INVALID                                        # NULL row set
    assert call([], nfields=-1) == INVALID                                      # nfields < 0
    assert call(None, nfields=1) == INVALID                                     # fields missing
    assert call([field()]) == INVALID                                           # none of the three pointers
    assert call([field(index=h1, column=h2)]) == INVALID                        # two of them
    assert call([field(index=h1, shards=h2)]) == INVALID
    assert call([field(shards=h1, column=h2)]) == INVALID
    assert call([field(index=h1, shards=h2, column=h3)]) == INVALID
    assert call([field(index=h1), field()]) == INVALID                          # the bad field is not the first
    assert call([field(column=h1, nkw=1)]) == INVALID                           # keywords on a column field
    assert call([field(index=h1, nkw=1, with_offsets=False)]) == INVALID        # keywords without offsets
    assert call([field(index=h1)], left=(None, 3)) == INVALID                   # lengths without bytes
    assert call([field(index=h1)], right=(None, 1)) == INVALID
    assert bytes(scratch.raw) == bytes(256)                                     # nothing wrote to the dummies either


def test_column_values_argument_checks(lib):
    scratch = C.create_string_buffer(64)
    col = C.c_void_p(C.addressof(scratch))
    ids = np.array([1, 2, 3], dtype=np.int64)
    values, found, missing = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint8), C.c_uint64(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.cdb_column_values(None, p(ids), 3, p(values), p(found), C.byref(missing)) == INVALID
    assert lib.cdb_column_values(col, None, 3, p(values), p(found), C.byref(missing)) == INVALID      # NULL ids with nrows > 0
    assert lib.cdb_column_values(col, p(ids), 3, None, p(found), C.byref(missing)) == INVALID
    assert lib.cdb_column_values(col, p(ids), 3, p(values), None, C.byref(missing)) == INVALID
    assert missing.value == 7 and bytes(scratch.raw) == bytes(64)


def test_selected_free_accepts_null_and_empty(lib):
    lib.cdb_selected_free(None)
    out = capi.CdbSelected()
    lib.cdb_selected_free(C.byref(out))
    assert _is_zeroed(out)


def test_shim_select_header_compiles_against_the_public_header():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no C++ compiler")
    r = subprocess.run([cxx, "-std=c++20", "-Wall", "-fsyntax-only", "-x", "c++", os.path.join(SHIM, "select.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
