"""CPU: the TX table's rules, host table and host form (route_core.hpp, route.cpp) under sanitizers
— tests/sanitize_route builds a stand-alone program with g++ (no HIP, nothing preloaded): the ASan +
UBSan build resolves every truncation of its packet templates from exact-size heap buffers and runs
random updates against a linear-scan model (and the threads once), the TSan build runs two updating
threads against two resolving ones and checks that a steady address never misses and that every
batch sees one route set as a whole."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan and libtsan")
def test_route_sanitizer_builds_run_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_route")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("route_test: ok (exact, threads)") == 1, r.stdout
    assert r.stdout.count("route_test: ok (threads)") == 1, r.stdout
