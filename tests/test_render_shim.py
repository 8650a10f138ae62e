"""string_index::render_rows through the reference-side binding (tests/cpp/test_render_shim.cpp): a database.cpp-style caller
renders a page, one id the index lacks included, and compares every string with cdb_shim::render_spans over highlight_spans."""
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
    exe = os.path.join(CPP, "test_render_shim")
    # the compile line tests/cpp/Makefile uses for the other shim programs
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_render_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"COFFEEDB_GPUS": "0,0", "COFFEEDB_SHARD_ALL": "1"}], ids=["one_gpu", "two_shards"])
def test_shim_render_rows_equals_render_spans(env):
    exe = _build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
