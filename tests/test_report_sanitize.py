"""CPU: the RX batch report's rules and host form (report_core.hpp, report.cpp) under sanitizers —
tests/sanitize_report builds a stand-alone program with g++ (no HIP, nothing preloaded): the ASan +
UBSan build runs the host form over every status x header x length, random batches and hostile ones
(lengths and offsets past the arena, entry indexes past from[]), every buffer a heap allocation of
exactly its length, against the per-packet walk restated in the program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_report_sanitizer_build_runs_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "sanitize_report")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("report_test: ok (directed, random, hostile)") == 1, r.stdout
