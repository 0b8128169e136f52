"""CPU: the TX send plan's rules and host form (send_core.hpp, send.cpp) under sanitizers —
tests/sanitize_send builds a stand-alone program with g++ (no HIP, nothing preloaded): the ASan +
UBSan build plans random batches from heap buffers of exactly their length into outputs of exactly
nwires elements, against the packing loop restated in the program, and runs send_core.hpp's
predicates composed as the device form composes them against the same loop."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_send_sanitizer_build_runs_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_send")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("send_test: ok (exact, parallel)") == 1, r.stdout
