"""CPU: the receive coalescer's rules and host form (coalesce_core.hpp, coalesce.cpp) under
ASan + UBSan — tests/sanitize_coalesce builds a stand-alone program with g++ (no HIP, nothing
preloaded) that fuzzes the parsers on exact-size buffers, runs a randomised batch and the capacity
cuts, and checks the results' invariants."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_coalesce_sanitizer_build_runs_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_coalesce")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("coalesce_test: ok") == 1, r.stdout
