"""The 16-byte edge record of the last pass over cells on the host alone (tests/cpp/test_seg_cell_edge.cpp): seg_cell_edge.h needs
no HIP, so a plain g++ program packs and unpacks records at the ends of every field and calls the two limit checks (output slots
below 2^48, runs of at most 16384 elements) on both sides of each limit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "coffeedb_amd", "csrc")


def test_edge_record_round_trips_and_limits(tmp_path):
    exe = str(tmp_path / "test_seg_cell_edge")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", f"-I{CSRC}",
                           os.path.join(CPP, "test_seg_cell_edge.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout[-4000:] + out.stderr[-2000:]
