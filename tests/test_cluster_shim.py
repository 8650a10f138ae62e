"""`cluster` through the reference-side binding with COFFEEDB_GPU_NUMERIC=1: string_index / integer_index / double_index /
bool_index::cluster against a literal restatement of database.cpp:442-460 (tests/cpp/test_cluster_shim.cpp, device part)."""
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
    exe = os.path.join(CPP, "test_cluster_shim")
    # the compile line tests/cpp/Makefile uses for the other shim programs
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_cluster_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


@pytest.mark.gpu
def test_shim_cluster_on_gpu_columns_and_string_index():
    exe = _build()
    env = dict(os.environ, COFFEEDB_GPU_NUMERIC="1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
