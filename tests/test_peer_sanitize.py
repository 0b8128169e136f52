"""CPU: the peer table's rules, host table and host form (peer_core.hpp, peer.cpp) under sanitizers —
tests/sanitize_peer builds a stand-alone program with g++ (no HIP, nothing preloaded): the ASan +
UBSan build resolves every truncation of its opened packets from exact-size heap buffers, runs
random updates against a linear-scan model and against the same records kept as a device image
through table_mirror.hpp on a fake device (and the threads once), the TSan build runs two updating
threads against two resolving ones and checks that a steady entry never misses and that a replaced
one is never absent."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan and libtsan")
def test_peer_sanitizer_builds_run_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_peer")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("peer_test: ok (exact, image, threads)") == 1, r.stdout
    assert r.stdout.count("peer_test: ok (threads)") == 1, r.stdout
