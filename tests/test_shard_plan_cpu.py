"""The planning arithmetic of a sharded column (coffeedb_amd/csrc/shard_plan.h: shard count, document-aligned bounds, the cuts of an
appended batch) as plain host code: tests/cpp/test_shard_plan.cpp is compiled on its own with the address and undefined-behaviour
sanitizers and run (no GPU, no library, nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_shard_plan_against_naive_restatements_under_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(ROOT, "coffeedb_amd", "csrc", "shard_plan.h")), "coffeedb_amd/csrc/shard_plan.h is missing"
    exe = str(tmp_path / "test_shard_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CPP, "test_shard_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
