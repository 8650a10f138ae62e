"""The reference-side binding with COFFEEDB_GPU_NUMERIC=1: bool / integer / double indexes backed by GPU columns, and a
device-side filter() through cdb_query_and_columns (tests/cpp/test_column_shim.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SHIM = os.path.join(ROOT, "coffeedb_amd", "csrc", "shim")
CSRC = os.path.join(ROOT, "coffeedb_amd", "csrc")


def _build():
    from coffeedb_amd import capi
    capi.build_library()
    exe = os.path.join(CPP, "test_column_shim")
    # the compile line of tests/cpp/Makefile
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_column_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


@pytest.mark.gpu
def test_shim_numeric_and_bool_indexes_on_gpu_columns():
    exe = _build()
    env = dict(os.environ, COFFEEDB_GPU_NUMERIC="1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
