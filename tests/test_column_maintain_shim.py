"""The reference-side binding with COFFEEDB_GPU_NUMERIC=1: append() of the bool / integer / double indexes hands the rows add()
collected since the last build() to cdb_column_append; without the variable (the CPU classes) it is false
(tests/cpp/test_column_maintain_shim.cpp)."""
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
    exe = os.path.join(CPP, "test_column_maintain_shim")
    # the compile line of tests/cpp/Makefile
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_column_maintain_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


def test_append_is_false_on_the_cpu_classes():
    exe = _build()
    env = {k: v for k, v in os.environ.items() if k != "COFFEEDB_GPU_NUMERIC"}
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_shim_append_on_gpu_columns():
    exe = _build()
    env = dict(os.environ, COFFEEDB_GPU_NUMERIC="1")
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
