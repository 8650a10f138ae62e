"""The error model of the C boundary on the host alone (tests/cpp/test_error_boundary.cpp): errors.h needs no HIP, so a plain
g++ program throws every kind of error and checks the code and the message the boundary would report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "coffeedb_amd", "csrc")


def test_status_comes_from_the_error_not_from_its_text(tmp_path):
    exe = str(tmp_path / "test_error_boundary")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-Wall", f"-I{CSRC}",
                           os.path.join(CPP, "test_error_boundary.cpp"), "-lpthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
