"""The keyword-list pieces of the query entry points (coffeedb_amd/csrc/keyword_list.h: the checks an entry point makes on its list,
the rebase onto the first byte, the rebase that drops empty keywords) as plain host code: tests/cpp/test_keyword_list.cpp is
compiled on its own with the address and undefined-behaviour sanitizers and run (no GPU, no library, nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_keyword_list_against_naive_restatements_under_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(ROOT, "coffeedb_amd", "csrc", "keyword_list.h")), "coffeedb_amd/csrc/keyword_list.h is missing"
    exe = str(tmp_path / "test_keyword_list")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(CPP, "test_keyword_list.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
