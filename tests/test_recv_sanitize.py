"""CPU: the RX receive plan's rules and host form (recv_core.hpp, recv.cpp) under sanitizers —
tests/sanitize_recv builds a stand-alone program with g++ (no HIP, nothing preloaded): the ASan +
UBSan build runs recv_core.hpp's cmsg walk and the host form over the directed control buffers and
random hostile ones, each at the very end of a heap allocation of exactly its length, and plans
random batches from exact-size heap buffers into exact-size outputs, against the loop restated in the
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_recv_sanitizer_build_runs_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_recv")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("recv_test: ok (walk, exact)") == 1, r.stdout
