"""CPU: the connection table's rules, host-only table and host forms (conntrack_core.hpp,
conntrack.cpp) under sanitizers — tests/sanitize_conntrack builds a stand-alone program with g++ (no
HIP, nothing preloaded): the ASan + UBSan build runs random batches of lookups, adds, evicts and
compactions from exact-size heap buffers against a linear-scan model (and the threads once), the
TSan build runs one adding and evicting thread against two looking-up ones and checks that a steady
key never misses and that a removed key never hits afterwards."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan and libtsan")
def test_conntrack_sanitizer_builds_run_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_conntrack")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("conntrack_test: ok (exact, threads)") == 1, r.stdout
    assert r.stdout.count("conntrack_test: ok (threads)") == 1, r.stdout
