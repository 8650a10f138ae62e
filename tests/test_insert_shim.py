"""cdb_shim::insert through the reference-side binding (tests/cpp/test_insert_shim.cpp): a database.cpp-style caller inserts objects
with two string fields, an integer, a double and a bool field in one call, gets the reference's three messages for an empty object,
an empty key and a value of the wrong type, the library's text for an id that is already held and for a failing field (after which
nothing has changed), and reads the inserted objects back by select."""
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
    exe = os.path.join(CPP, "test_insert_shim")
    # the compile line tests/cpp/Makefile uses for the other shim programs
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_insert_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


def test_shim_program_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_shim_insert_equals_the_model():
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, COFFEEDB_GPU_NUMERIC="1"))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
