"""The k-way merge of per-shard cluster groups (coffeedb_amd/csrc/cluster_merge.h) as plain host code: tests/cpp/test_cluster_merge.cpp
is compiled on its own with the address and undefined-behaviour sanitizers and run (no GPU, no library, nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_cluster_merge_against_std_map_under_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(ROOT, "coffeedb_amd", "csrc", "cluster_merge.h")), "coffeedb_amd/csrc/cluster_merge.h is missing"
    exe = str(tmp_path / "test_cluster_merge")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CPP, "test_cluster_merge.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
