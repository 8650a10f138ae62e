"""The alphabetic code of the bucket-wise build's sort keys on the host alone (tests/cpp/test_vl_code.cpp): vl_code.h needs no HIP,
so a plain g++ program builds codes over skewed, sparse and depth-limit-forcing counts and checks that each is order-preserving,
prefix-free and complete, that the sweep's tables decode it, and how far it lies from the optimal alphabetic tree."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "coffeedb_amd", "csrc")


def test_codes_are_alphabetic_complete_and_near_optimal(tmp_path):
    exe = str(tmp_path / "test_vl_code")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", f"-I{CSRC}",
                           os.path.join(CPP, "test_vl_code.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout[-4000:] + out.stderr[-2000:]
