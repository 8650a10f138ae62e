"""cdb_shim::select through the reference-side binding (tests/cpp/test_select_shim.cpp): a database.cpp-style caller with two
string fields, an int64 field and a bool field over some twenty objects with differing field sets runs the README's query shapes
and compares every answer with database.cpp:394-441 restated over its own std::map objects — on one GPU and with the string
fields sharded."""
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
    exe = os.path.join(CPP, "test_select_shim")
    # the compile line tests/cpp/Makefile uses for the other shim programs
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_select_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"COFFEEDB_GPUS": "0,0", "COFFEEDB_SHARD_ALL": "1"}], ids=["one_gpu", "two_shards"])
def test_shim_select_equals_the_reference_rules(env):
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, COFFEEDB_GPU_NUMERIC="1", **env))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
