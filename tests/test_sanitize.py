"""CPU: the engine's host logic under sanitizers — `make -C nebula_amd sanitize`
builds window_core.hpp (replay window, exact receive rounds, thread pool) and queue_core.hpp (the
submission queue, on a CPU device running the oracle) and workspace.hpp (the device workspaces'
event and stream protocol, on a fake device that logs the calls) and hip_owned.hpp (the owned
buffers' growth, moves and release, on such a fake too) and table_mirror.hpp (the lookup tables'
two device images, staging and events, on such a fake too) and comb_core.hpp (the per-packet
combiner's leader/joiner protocol, on a fake device whose launches the test holds and releases)
and pipe_core.hpp (the staged host
pipeline's chunk plan, chunk spans and overlap test, against brute force) with ASan+UBSan and with
TSan and runs them; the first two also check their results against the packet-by-packet receive /
the oracle."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan/libtsan")
def test_sanitizer_builds_run_clean():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "nebula_amd"), "sanitize"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("window_test: ok") == 2 and r.stdout.count("queue_test: ok") == 2, r.stdout
    assert r.stdout.count("workspace_test: ok") == 2, r.stdout
    assert r.stdout.count("pipe_test: ok") == 2, r.stdout
    assert r.stdout.count("owned_test: ok") == 2, r.stdout
    assert r.stdout.count("mirror_test: ok") == 2, r.stdout
    assert r.stdout.count("comb_test: ok") == 2, r.stdout
