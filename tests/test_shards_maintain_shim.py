"""`cluster`, `remove` and `append` of a sharded string column through the reference-side binding: string_index with
COFFEEDB_GPUS="0,0" (two shards on device 0) against a literal restatement of database.cpp:442-460 and against freshly built
indexes (tests/cpp/test_shards_maintain_shim.cpp)."""
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
    exe = os.path.join(CPP, "test_shards_maintain_shim")
    # the compile line tests/test_cluster_shim.py uses
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{SHIM}", os.path.join(CPP, "test_shards_maintain_shim.cpp"),
                           os.path.join(SHIM, "index.cpp"), f"-L{CSRC}", "-lcoffeedb_gpu", f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib",
                           "-lpthread", "-o", exe])
    return exe


@pytest.mark.gpu
def test_shim_cluster_remove_append_on_a_sharded_string_index():
    exe = _build()
    env = dict(os.environ, COFFEEDB_GPUS="0,0", COFFEEDB_SHARD_ALL="1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
