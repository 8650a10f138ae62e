"""cdb_shim::rowset::remove and rowset::everything through the reference-side binding (tests/cpp/test_rowset_maintain_shim.cpp): a
database.cpp-style caller removes by constraints over two string fields and an integer field in one call, counts and queries (with
`span` and fields) without constraints, and gets a failing field rethrown as std::runtime_error with the library's text — every
answer compared with the same operation over its own std::map objects."""
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
    exe = os.path.join(CPP, "test_rowset_maintain_shim")
    # the compile line tests/cpp/Makefile uses for the other shim programs
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_rowset_maintain_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


def test_shim_program_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_shim_remove_and_everything_equal_the_model():
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, COFFEEDB_GPU_NUMERIC="1"))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
