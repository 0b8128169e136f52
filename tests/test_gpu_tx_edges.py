"""GPU: the directed transmit cases (tests/tx_cases.py; what they reach is pinned on the CPU by
tests/test_tx_cases.py) through every form of the transmit batch: every wire byte, wire record,
status and final counter against segment_oracle.tx_batch, and through a relay against
tx_via_ref.tx_via_batch. The reads lie at byte skews 0..15, rotated from run to run."""
import random

import numpy as np
import pytest

import tx_cases as T
import tx_via_ref as M
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

import test_gpu_tx_via as V  # noqa: E402
from test_gpu_tx import _check, _to_arrays, _tunnels  # noqa: E402

OUT_CAP, MAX_WIRES = 4 << 20, 4096


@pytest.fixture(scope="module")
def cases():
    return T.cases()


def _direct(engine, oracle_mod, alg, cases, ntun, rotation, **kw):
    reads, skews = T.batch(cases, ntun, rotation)
    tun = _tunnels(random.Random(100 + rotation), n=ntun, keyless=())
    return _check(engine, oracle_mod, alg, reads, tun, out_cap=OUT_CAP, max_wires=MAX_WIRES, skew=skews, **kw)


@pytest.mark.parametrize("device", [False, True])
def test_edges_gcm_three_keys(engine, oracle_mod, cases, device):
    """The segment kernel sums every payload; the chunk kernel seals."""
    r = _direct(engine, oracle_mod, L.ALG_AESGCM, cases, 3, T.ROTATIONS[device], device=device)
    assert (r.wire_status == L.STATUS_OK).all()


@pytest.mark.parametrize("grid", [None, 1])
def test_edges_gcm_one_key(engine, oracle_mod, cases, grid, knobs):
    """key_hint: the CSM segment kernel, the seal sums the payloads of the segments seal_cs admits.
    With a 1-workgroup seal grid the wires past its last full pass of 256 go to the tail kernel and
    are summed by the segment kernel."""
    if grid is not None:
        knobs(L.KNOB_SINGLE_MAX_GRID, grid)
    r = _direct(engine, oracle_mod, L.ALG_AESGCM, cases, 1, T.ROTATIONS[2 + (grid is not None)], key_hint=0)
    if grid is not None:
        assert len(r.wires) > 256 and len(r.wires) % 256 != 0


@pytest.mark.parametrize("device", [False, True])
def test_edges_chacha_three_keys(engine, oracle_mod, cases, device):
    _direct(engine, oracle_mod, L.ALG_CHACHAPOLY, cases, 3, T.ROTATIONS[4 - device], device=device)


class _SharedKeys(V._Keys):
    """test_gpu_tx_via._Keys with one installed key for all tunnels of equal key bytes, so that two
    tunnels can run under the one key a key_hint names."""

    def __init__(self, engine, alg, tun_spec):
        from nebula_amd.inside import TX_TUNNEL_DTYPE
        from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

        cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
        self.owned = {}
        for t in tun_spec:
            if t["key"] not in self.owned:
                self.owned[t["key"]] = cf.Cipher(engine, t["key"])
        self.ciphers = [self.owned[t["key"]] for t in tun_spec]
        self.tun = np.zeros(len(tun_spec), TX_TUNNEL_DTYPE)
        for i, (t, c) in enumerate(zip(tun_spec, self.ciphers)):
            self.tun[i] = (t["counter"], c.key_id, t["remote_index"])

    def close(self):
        for c in self.owned.values():
            c.destroy()


def _via(engine, oracle_mod, cases, keys, rotation, key_hint, monkeypatch):
    """Tunnel 0 is the relay; of the other tunnels the first half go through it and the rest
    directly. keys: the tunnels' keys."""
    n = len(keys) - 1
    reads, skews = T.batch(cases, n, rotation)
    reads = [dict(p, tunnel=p["tunnel"] + 1) for p in reads]
    tun = [dict(counter=5 + 3000 * t, remote_index=0xB000 + t, key=k) for t, k in enumerate(keys)]
    via = [(M.RELAY_NONE, 0)] + [(0, 0x7000 + t) if t <= n // 2 else (M.RELAY_NONE, 0) for t in range(1, n + 1)]
    monkeypatch.setattr(V, "_Keys", _SharedKeys)
    r, exp_w = V._check(engine, oracle_mod, L.ALG_AESGCM, reads, tun, via, out_cap=OUT_CAP, max_wires=MAX_WIRES,
                        device=True, key_hint=key_hint, skew=skews)
    nvia = int((r.wires["reserved"] == L.TX_WIRE_VIA).sum())
    assert 0 < nvia < len(r.wires)
    return r


def test_edges_via_mixed_keys(engine, oracle_mod, cases, monkeypatch):
    rng = random.Random(7)
    _via(engine, oracle_mod, cases, [rng.randbytes(32) for _ in range(5)], T.ROTATIONS[1], None, monkeypatch)


def test_edges_via_one_target_key(engine, oracle_mod, cases, monkeypatch):
    """tx_segment_kernel<CSM, VIA>: one relay, and two tunnels under the one key the hint names, one
    of them through the relay."""
    rng = random.Random(8)
    k_relay, k_target = rng.randbytes(32), rng.randbytes(32)
    _via(engine, oracle_mod, cases, [k_relay, k_target, k_target], T.ROTATIONS[3], 1, monkeypatch)


@pytest.mark.parametrize("alg,single", [(L.ALG_AESGCM, False), (L.ALG_AESGCM, True), (L.ALG_CHACHAPOLY, False)])
def test_steered_zero_checksums_on_the_wire(engine, oracle_mod, cases, alg, single):
    """The steered reads alone: every wire opens under its tunnel's key, and the L4 checksum field of
    each steered segment is 0xFFFF for UDP (RFC 768: a computed zero is sent as all ones) and 0x0000
    for TCP, which has no such rule."""
    from nebula_amd.inside import TX_TUNNEL_DTYPE, tx_seal_batch_host
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

    reads = T.steered(cases)
    ntun = 1 if single else 3
    reads = [dict(p, tunnel=i % ntun) for i, p in enumerate(reads)]
    spec = _tunnels(random.Random(3), n=ntun, keyless=())
    cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
    ciphers = [cf.Cipher(engine, t["key"]) for t in spec]
    try:
        tun = np.zeros(ntun, TX_TUNNEL_DTYPE)
        for i, (t, c) in enumerate(zip(spec, ciphers)):
            tun[i] = (t["counter"], c.key_id, t["remote_index"])
        pk, arena = _to_arrays(reads, [3, 8, 0, 13, 6, 1, 10])
        r = tx_seal_batch_host(engine, alg, tun, pk, arena, 1 << 18, 256, ciphers[0].key_id if single else L.KEYS_MIXED)
    finally:
        for c in ciphers:
            c.destroy()
    assert (r.packet_status == L.STATUS_OK).all() and len(r.wires) == 4 * 4 + 3 and (r.wire_status == L.STATUS_OK).all()
    steered = {"udp": 0, "tcp": 0, "finish": 0}
    for i, w in enumerate(r.wires):
        p, j = reads[int(w["packet"])], int(w["segment"])
        b = r.wire_bytes(i)
        seg = oracle_mod.open_(alg, spec[p["tunnel"]]["key"], oracle_mod.nonce(alg, int(w["counter"])), b[:16], b[16:])
        assert seg is not None, f"wire {i} does not authenticate"
        kind, f = T.kind_of(p), T.field_of(p)
        if kind != "finish" and j == 2:
            continue  # the one segment of each superpacket that was not steered
        udp = kind == "udp" or (kind == "finish" and p["csum_offset"] == 6)
        got = int.from_bytes(seg[f:f + 2], "big")
        assert T.computed_l4(p, seg) == 0, (kind, j)
        if udp:
            assert got == 0xFFFF, f"UDP computed zero must go out as 0xFFFF, got {got:#06x} ({kind}, segment {j})"
        else:
            assert got == 0x0000, f"TCP computed zero must stay 0x0000, got {got:#06x} ({kind}, segment {j})"
        steered[kind] += 1
    assert steered == {"udp": 6, "tcp": 6, "finish": 3}
