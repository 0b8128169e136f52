"""CPU: the TX-through-a-relay entry points exist in the ABI and the binding, and the sequential
model the GPU tests compare against (tests/tx_via_ref.py) checks itself against
segment_oracle.tx_batch, the relay forwarding model and the oracle's open. No GPU."""
import os
import random
import re

import numpy as np

import relay_forward_ref as F
import tx_via_ref as M
from nebula_amd import _lib as L
from test_gpu_tx import _mixed_packets, _pk, _tunnels
from test_segment_oracle import build_tcpv4_super

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGS = [L.ALG_AESGCM, L.ALG_CHACHAPOLY]


def test_tx_via_symbols_and_binding():
    lib = L.lib()
    for s in ("neb_tx_seal_via_batch", "neb_tx_seal_via_batch_host"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    text = open(os.path.join(ROOT, "include", "nebula_aead.h")).read()
    assert int(re.search(r"#define NEB_TX_WIRE_VIA (\d+)", text).group(1)) == L.TX_WIRE_VIA == 1
    from nebula_amd import inside

    assert callable(inside.tx_seal_via_batch_host) and "tx_seal_via_batch_host" in inside.__all__
    assert [inside.slot_bytes_via(n) for n in (0, 1, 16, 17)] == [64, 80, 80, 96]
    assert all(inside.slot_bytes_via(n) == inside.slot_bytes(n) + 32 == M.slot_bytes_via(n) for n in range(200))
    # bad arguments are refused before any device work
    assert lib.neb_tx_seal_via_batch(None, 1, None, 0, None, None, 0, None, None, 0, None, None, 0, None, None,
                                     L.KEYS_MIXED, None) == L.ERR_INVALID
    assert lib.neb_tx_seal_via_batch_host(None, 1, None, 0, None, None, 0, None, 0, None, 0, None, None, 0, None, None,
                                          L.KEYS_MIXED) == L.ERR_INVALID


def test_model_without_relays_is_the_direct_model(oracle_mod):
    import segment_oracle as S

    seal = M.oracle_seal(oracle_mod)
    for alg in ALGS:
        for out_cap, max_wires in ((1 << 20, 4096), (9000, 4096), (1 << 20, 7)):
            rng = random.Random(alg)
            P, tun = _mixed_packets(S, rng), _tunnels(rng)
            want = S.tx_batch(alg, tun, P, out_cap, max_wires, seal, oracle_mod.header_encode)
            for via in (None, [(M.RELAY_NONE, 7)] * len(tun)):
                w, pst, ctr = M.tx_via_batch(alg, tun, via, P, out_cap, max_wires, seal, oracle_mod.header_encode)
                assert (pst, ctr) == want[1:]
                assert [x[:6] + x[7:] for x in w] == want[0] and all(x[6] == 0 for x in w)


def _via_case(oracle_mod, alg):
    """Two reads (a 3-segment TSO superpacket with a short last segment, a plain packet) of tunnel 0,
    which is reached through tunnel 1."""
    import segment_oracle as S

    rng = random.Random(100 + alg)
    tun = _tunnels(rng, n=2, keyless=())
    tcp, _, cs = build_tcpv4_super(2500)
    P = [_pk(tcp, 0, 1, S.GSO_TCPV4, 1000, cs, 16), _pk(bytes(rng.getrandbits(8) for _ in range(77)), 0)]
    via = [(1, 0xBEEF), (M.RELAY_NONE, 0)]
    seal = M.oracle_seal(oracle_mod)
    got = M.tx_via_batch(alg, tun, via, P, 1 << 20, 64, seal, oracle_mod.header_encode)
    direct = S.tx_batch(alg, tun, P, 1 << 20, 64, seal, oracle_mod.header_encode)
    return S, tun, P, via, got, direct


def test_model_via_wire_wraps_the_direct_wire(oracle_mod):
    for alg in ALGS:
        S, tun, P, via, (w, pst, ctr), (dw, dpst, dctr) = _via_case(oracle_mod, alg)
        assert pst == dpst == [0, 0] and len(w) == len(dw) == 4
        assert ctr == [tun[0]["counter"] + 4, tun[1]["counter"] + 4] and dctr[1] == tun[1]["counter"]
        off = 0
        for k, (x, d) in enumerate(zip(w, dw)):
            assert x[:6] == (off, d[1], d[2] + 32, d[3], d[4], S.OK) and x[6] == 1
            assert x[7][16:-16] == d[6]  # the inner bytes are the direct wire of the same counter
            r = tun[1]["counter"] + 1 + k
            assert x[7][:16] == oracle_mod.header_encode(1, 1, 1, 0xBEEF, r)
            assert oracle_mod.open_(alg, tun[1]["key"], oracle_mod.nonce(alg, r), x[7][:-16], x[7][-16:]) == b""
            off += M.slot_bytes_via(d[2] - 32)


def test_model_via_wire_is_forwarded_and_opens_at_the_target(oracle_mod):
    """The relay node's model (relay_forward_ref.forward) verifies each via wire under the relay
    tunnel's key and forwards it; the result opens under the target's key to the segment."""
    import replay_oracle as R

    for alg in ALGS:
        S, tun, P, via, (w, _, _), _ = _via_case(oracle_mod, alg)
        SL = 1200
        arena = np.zeros(SL * len(w), np.uint8)
        packets = []
        for i, x in enumerate(w):
            arena[i * SL:i * SL + x[2]] = list(x[7])
            packets.append((i * SL, x[2], 0))
        out_key = bytes(range(7, 39))
        status, fwd, exp, _, ctr = F.forward(oracle_mod, R, alg, [tun[1]["key"]], arena, packets,
                                             [(0, 0x51)] * len(w), [(500, out_key)], 2048, seen=())
        assert status == [R.OK] * 4 and fwd == [R.OK] * 4 and ctr == [504]
        segs = [s for p in P for s in S.segment_superpacket(p["data"], p["flags"], p["gso_type"], p["hdr_len"],
                                                            p["gso_size"], p["csum_start"], p["csum_offset"])]
        for i, (x, seg) in enumerate(zip(w, segs)):
            out = bytes(exp[i * SL:i * SL + x[2]])
            assert oracle_mod.open_(alg, out_key, oracle_mod.nonce(alg, 501 + i), out[:-16], out[-16:]) == b""
            inner = out[16:-16]
            assert inner[:16] == oracle_mod.header_encode(1, 1, 0, tun[0]["remote_index"], x[1])
            assert oracle_mod.open_(alg, tun[0]["key"], oracle_mod.nonce(alg, x[1]), inner[:16], inner[16:]) == seg


def test_model_relay_rules_and_exhaustion(oracle_mod):
    alg = L.ALG_AESGCM
    seal = M.oracle_seal(oracle_mod)
    rng = random.Random(3)
    tun = _tunnels(rng, n=6, keyless=(3,))
    via = [(M.RELAY_NONE, 0), (0, 1), (3, 2), (9, 3), (1, 4), (5, 5)]
    P = [_pk(b"p" * 30, t) for t in (0, 1, 2, 3, 4, 5, 1)]
    w, pst, ctr = M.tx_via_batch(alg, tun, via, P, 1 << 20, 64, seal, oracle_mod.header_encode)
    # direct; via 0; via keyless 3; keyless target (its via out of range); via 1, which has a via; via itself
    assert pst == [0, 0, 3, 3, 5, 5, 0]
    assert [(x[3], x[6]) for x in w] == [(0, 0), (1, 1), (6, 1)]
    base = [t["counter"] for t in tun]
    assert ctr == [base[0] + 3, base[1] + 2] + base[2:]
    # the target at REJECT_AFTER - 3: four exhausted inner counters take no outer one
    for who, want in ((1, [6, 2]), (0, [6, 6])):
        t2 = [dict(t) for t in tun[:2]]
        t2[who]["counter"] = M.S.REJECT_AFTER - 3
        start = [t["counter"] for t in t2]
        w, pst, ctr = M.tx_via_batch(alg, t2, [(M.RELAY_NONE, 0), (0, 1)], [_pk(b"q" * 9, 1)] * 6, 1 << 20, 64, seal,
                                     oracle_mod.header_encode)
        assert [x[5] for x in w] == [0, 0, 2, 2, 2, 2] and [x[7] is None for x in w] == [False] * 2 + [True] * 4
        assert [ctr[1] - start[1], ctr[0] - start[0]] == want
