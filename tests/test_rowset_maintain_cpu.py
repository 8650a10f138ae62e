"""cdb_rowset_remove / cdb_rowset_all without a GPU: both symbols are declared, exported and listed; null and negative arguments
answer CDB_E_INVALID and leave *out null; cdb_remove_field has the layout the C compiler gives it; without a device the answer is
CDB_E_DEVICE (the handles given are zeroed scratch memory of which only the device number may be read); shim/rowset.h still compiles
against the public header; and the numpy referee of the union (tests/rowset_all_referee.py) agrees with Python's own sorted(set())."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from coffeedb_amd import capi

from . import rowset_all_referee as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "coffeedb_gpu.h")
NEW = ["cdb_rowset_remove", "cdb_rowset_all"]
INVALID, DEVICE = 1, 2
FIELDS = ["index", "column", "removed", "missing", "status", "committed"]


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
        assert not re.search(r"[^a-z_]", name)
    assert lib.cdb_rowset_remove.argtypes[1]._type_ is capi.CdbRemoveField


def test_remove_field_layout_as_stated():
    """LP64: two pointers, two uint64_t, two int32_t — 40 bytes without padding"""
    cls = capi.CdbRemoveField
    assert [f for f, _ in cls._fields_] == FIELDS
    assert (C.sizeof(cls), [getattr(cls, f).offset for f in FIELDS]) == (40, [0, 8, 16, 24, 32, 36])


def test_remove_field_layout_equals_the_c_compilers(tmp_path):
    cc = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             '    printf("%zu", sizeof(cdb_remove_field));']
    lines += [f'    printf(" %zu", offsetof(cdb_remove_field, {f}));' for f in FIELDS]
    lines += ['    printf("\\n");', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])   # (the header is plain C)
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    cls = capi.CdbRemoveField
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f in FIELDS]


def _field(index=None, column=None):
    f = capi.CdbRemoveField()
    f.index, f.column = index, column
    f.removed, f.missing, f.status, f.committed = 11, 12, 13, 14
    return f


def test_rowset_remove_argument_checks(lib):
    """None of these may read the row set or a field's handle: the handles are addresses inside a scratch buffer."""
    scratch = C.create_string_buffer(256)
    rs, h1, h2 = (C.c_void_p(C.addressof(scratch) + 64 * k) for k in range(3))
    rows = C.c_uint64(99)

    def call(fields, nfields=None, rs_=rs):
        arr = (capi.CdbRemoveField * max(len(fields), 1))(*fields) if fields is not None else None
        rows.value = 99
        rc = lib.cdb_rowset_remove(rs_, arr, len(fields) if nfields is None else nfields, C.byref(rows))
        assert rows.value == 0
        return rc

    assert call([_field(index=h1)], rs_=None) == INVALID          # NULL row set
    assert call(None, nfields=1) == INVALID                        # fields missing
    assert call([], nfields=0) == INVALID                          # nfields < 1
    assert call([_field(index=h1)], nfields=-1) == INVALID
    assert call([_field()]) == INVALID                             # neither pointer
    assert call([_field(index=h1, column=h2)]) == INVALID          # both
    assert call([_field(index=h1), _field()]) == INVALID           # the bad entry is not the first
    assert call([_field(index=h1), _field(index=h1)]) == INVALID   # the same handle twice
    assert call([_field(column=h2), _field(index=h1), _field(column=h2)]) == INVALID
    assert lib.cdb_rowset_remove(None, None, 0, None) == INVALID   # (rows may be NULL)
    assert bytes(scratch.raw) == bytes(256)


def test_rowset_all_argument_checks(lib):
    scratch = C.create_string_buffer(128)
    h1 = C.addressof(scratch)
    one = (C.c_void_p * 1)(h1)
    null = (C.c_void_p * 2)(h1, None)
    out = C.c_void_p(7)

    def call(idx, ni, cols, nc, o=out):
        out.value = 7
        rc = lib.cdb_rowset_all(idx, ni, cols, nc, C.byref(o) if o is not None else None)
        assert o is None or not out.value, "*out stays null"
        return rc

    assert call(one, 1, None, 0, o=None) == INVALID        # NULL out
    assert call(None, 0, None, 0) == INVALID               # no field at all
    assert call(one, -1, None, 0) == INVALID               # negative counts
    assert call(None, 0, one, -1) == INVALID
    assert call(one, 1, one, -1) == INVALID
    assert call(None, 1, None, 0) == INVALID               # a count without its array
    assert call(None, 0, None, 2) == INVALID
    assert call(null, 2, None, 0) == INVALID               # a null entry
    assert call(None, 0, null, 2) == INVALID
    assert bytes(scratch.raw) == bytes(128)
    with pytest.raises(TypeError):
        capi.rowset_all([object()])
    with pytest.raises(RuntimeError, match="no field given"):
        capi.rowset_all([])


def test_no_device_answer(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    big = C.create_string_buffer(1 << 20)   # zeroed: device 0; nothing else of a handle may be read before the device is known
    h = (C.c_void_p * 1)(C.addressof(big))
    out = C.c_void_p(7)
    assert lib.cdb_rowset_all(h, 1, None, 0, C.byref(out)) == DEVICE and not out.value
    out.value = 7
    assert lib.cdb_rowset_all(None, 0, h, 1, C.byref(out)) == DEVICE and not out.value
    f = (capi.CdbRemoveField * 1)(_field(index=C.addressof(big) + (1 << 19)))
    rows = C.c_uint64(5)
    assert lib.cdb_rowset_remove(C.c_void_p(C.addressof(big)), f, 1, C.byref(rows)) == DEVICE
    assert (rows.value, f[0].removed, f[0].missing, f[0].status, f[0].committed) == (0, 0, 0, 0, 0)
    assert bytes(big.raw) == bytes(1 << 20)


def test_shim_header_compiles_against_the_public_header():
    shim = os.path.join(ROOT, "coffeedb_amd", "csrc", "shim", "rowset.h")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-x", "c++", shim])


def test_union_referee_agrees_with_python_sorted_set():
    lo, hi = -(1 << 63), (1 << 63) - 1
    rng = np.random.default_rng(20261020)
    lists = [np.array([hi, 0, -1, lo, 5, 7], dtype=np.int64), np.array([-1, 0, 3, lo], dtype=np.int64), np.empty(0, dtype=np.int64),
             rng.integers(-50, 50, 300).astype(np.int64), np.array([hi, hi - 1, lo + 1], dtype=np.int64)]
    for k in range(1, len(lists) + 1):
        got = R.union(lists[:k])
        want = sorted(set(x for l in lists[:k] for x in l.tolist()))
        assert got.dtype == np.int64 and got.tolist() == want
    full = R.union(lists)
    assert full[0] == lo and full[-1] == hi and (np.diff(full.astype(object)) > 0).all()   # negative ids first, each id once
    assert list(full).index(-1) < list(full).index(0)
    assert R.union([]).tolist() == [] and R.union([lists[2]]).tolist() == []
    ids, counts = R.page(full, 2, 5)
    assert ids.tolist() == full[2:5].tolist() and counts.tolist() == [0, 0, 0]
    assert R.page(full, 4, 4)[0].tolist() == [] and R.page(full, len(full) - 1, 10**9)[0].tolist() == [hi]
