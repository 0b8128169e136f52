"""CPU: the index table's rules, host table and host form (index_core.hpp, index.cpp) under
sanitizers — tests/sanitize_index builds a stand-alone program with g++ (no HIP, nothing preloaded):
the ASan + UBSan build runs random updates and the host resolve on exact-size buffers, del + put +
re-put calls slot by slot against a linear-scan model across the rebuild threshold (and the
threads once), the TSan build runs four updating threads against two resolving ones and checks that
a steady key never misses."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan and libtsan")
def test_index_sanitizer_builds_run_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_index")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("index_test: ok (exact, threads)") == 1, r.stdout
    assert r.stdout.count("index_test: ok (threads)") == 1, r.stdout
