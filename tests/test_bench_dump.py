"""GPU: bench.py --dump-outputs. dump_outputs() writes what the timed path's last step left (status,
opened slots) and what its seal wrote (tags, sealed slots) as float32 .npy files; here on a small
IMIX batch against the oracle, whole and through the fixed sample, and twice for determinism.
CPU: the option's parsing (refused outside the device mode)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nebula_amd import _lib as L
from nebula_amd import workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [False, True])
def test_dump_outputs_match_oracle(engine, oracle_mod, tmp_path, monkeypatch, sample):
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from nebula_amd.batch import DeviceBatch, install_keys

    if sample:  # fewer than the batch holds: the seeded sample
        monkeypatch.setattr(bench, "DUMP_SLOTS", 37)
        monkeypatch.setattr(bench, "DUMP_TAGS", 101)
    b = W.make_batch(L.ALG_AESGCM, 333, 5, sizes=(90, 576, 1300), ratio=(7, 4, 1), name="dump")
    sealed = b.arena.copy()
    assert (oracle_mod.batch(b.alg, 0, b.keys, b.desc, sealed) == 0).all()
    opened = sealed.copy()
    assert (oracle_mod.batch(b.alg, 1, b.keys, b.desc, opened) == 0).all()
    ciphers = install_keys(engine, b)
    try:
        db = DeviceBatch(engine, b, ciphers)
        db.seal()
        db.open()
        torch.cuda.synchronize()
        st = db.status_host()
        after_step = db.arena_host()
        outs = []
        for k in range(2):
            bench.dump_outputs(str(tmp_path / f"d{k}"), db, st, 0)
            outs.append(_load(tmp_path / f"d{k}"))
        assert np.array_equal(db.arena_host(), after_step)  # the dump leaves the arena as the step left it
    finally:
        for c in ciphers:
            c.destroy()
    a, a2 = outs
    assert sorted(a) == ["opened_slots", "sealed_slots", "sealed_tags", "status"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[k], a2[k]) for k in a)
    rng = np.random.default_rng(bench.DUMP_SEED)  # the sample dump_outputs documents
    si = np.sort(rng.choice(b.n, 37, replace=False)) if sample else np.arange(b.n)
    ti = np.sort(rng.choice(b.n, 101, replace=False)) if sample else np.arange(b.n)
    assert np.array_equal(a["status"], np.zeros(b.n, np.float32))
    assert np.array_equal(a["sealed_slots"], sealed.reshape(b.n, b.stride)[si].astype(np.float32))
    assert np.array_equal(a["opened_slots"], after_step.reshape(b.n, b.stride)[si].astype(np.float32))
    lens = b.desc["len"].astype(np.int64)
    for row, i in zip(a["sealed_tags"], ti):
        assert np.array_equal(row, sealed.reshape(b.n, b.stride)[i, 16 + lens[i]:32 + lens[i]].astype(np.float32))
    # the opened arena holds the oracle's plaintext over every packet's header and payload
    ref_o = opened.reshape(b.n, b.stride)
    for row, i in zip(a["opened_slots"], si):
        assert np.array_equal(row[:16 + lens[i]], ref_o[i, :16 + lens[i]].astype(np.float32))


def test_dump_outputs_refused_outside_device_mode(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--dump-outputs", str(tmp_path / "x")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "x").exists()
