"""`cluster` without a GPU: the new C-ABI symbols (declared, exported, listed), their argument checks, and the host half of the
reference-side binding (coffeedb_amd/csrc/shim/cluster.h) — the strings std::to_string makes of the device's group values,
merged and ordered as database.cpp:442-460's std::map does — compiled into the host part of tests/cpp/test_cluster_shim.cpp."""
import ctypes as C
import os
import re
import subprocess

import pytest

from coffeedb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cdb_column_cluster", "cdb_cluster", "cdb_clusters_free")
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
    for field in ("ngroups", "missing", "counts", "rep_ids", "values", "value_ptr", "value_blob"):
        assert re.search(r"\b%s;" % field, header.split("typedef struct cdb_clusters")[1].split("cdb_clusters;")[0])
    assert [f[0] for f in capi.CdbClusters._fields_] == ["ngroups", "missing", "counts", "rep_ids", "values", "value_ptr", "value_blob"]
    assert C.sizeof(capi.CdbClusters) == 56


def test_null_arguments_are_invalid_without_a_device(lib):
    out = capi.CdbClusters()
    ids = (C.c_int64 * 2)(1, 2)
    fake = C.c_void_p(0)
    assert lib.cdb_column_cluster(None, ids, 2, C.byref(out)) == CDB_E_INVALID
    assert lib.cdb_cluster(None, ids, 2, 1, C.byref(out)) == CDB_E_INVALID
    assert lib.cdb_cluster(fake, ids, 2, 1, None) == CDB_E_INVALID
    assert lib.cdb_column_cluster(fake, ids, 2, None) == CDB_E_INVALID
    lib.cdb_clusters_free(None)
    zero = capi.CdbClusters()
    lib.cdb_clusters_free(C.byref(zero))   # an all-zero struct is released like any other
    assert zero.ngroups == 0 and not zero.counts


def test_shim_prints_merges_and_orders_like_the_reference(tmp_path):
    exe = os.path.join(str(tmp_path), "test_cluster_shim_host")
    shim = os.path.join(ROOT, "coffeedb_amd", "csrc", "shim")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", "-Werror", "-DCLUSTER_SHIM_HOST_ONLY", f"-I{shim}",
                           os.path.join(ROOT, "tests", "cpp", "test_cluster_shim.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
