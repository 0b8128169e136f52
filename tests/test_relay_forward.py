"""CPU: the relay forwarding entry points exist in the ABI and the binding, and the sequential
model the GPU tests compare against (tests/relay_forward_ref.py) checks itself against the oracle's
seal / open. No GPU."""
import random
import re
import os

import numpy as np

import relay_forward_ref as M
from nebula_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relay_forward_symbols_and_route_layout():
    lib = L.lib()
    for s in ("neb_relay_forward_batch", "neb_relay_forward_batch_host"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    assert L.RELAY_ROUTE_DTYPE.itemsize == 8  # sizeof(neb_relay_route)
    assert L.RELAY_ROUTE_DTYPE.names == ("tunnel", "remote_index")
    text = open(os.path.join(ROOT, "include", "nebula_aead.h")).read()
    assert int(re.search(r"#define NEB_STATUS_NOT_FORWARDED (\d+)", text).group(1)) == L.STATUS_NOT_FORWARDED == 8
    assert int(re.search(r"#define NEB_RELAY_NONE (\w+?)u?\n", text).group(1), 0) == L.RELAY_NONE == 0xFFFFFFFF
    import nebula_amd

    assert callable(nebula_amd.relay_forward_batch) and callable(nebula_amd.relay_forward_batch_device)
    # bad arguments are refused before any device work
    assert lib.neb_relay_forward_batch(None, 1, None, None, None, 0, None, 0, None, None, None, L.KEYS_MIXED,
                                       None) == L.ERR_INVALID
    assert lib.neb_relay_forward_batch_host(None, 1, None, 0, None, None, 0, None, 0, None, 0, None, None,
                                            L.KEYS_MIXED) == L.ERR_INVALID


def _model_case(oracle_mod, alg):
    import replay_oracle as R

    rng = random.Random(alg)
    key_a, key_b = (bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(2))
    inners = [bytes(rng.getrandbits(8) for _ in range(n)) for n in (0, 1, 16, 100)]
    SL = 256
    arena = np.zeros(SL * len(inners), np.uint8)
    packets, routes = [], []
    for i, inner in enumerate(inners):
        pkt = M.seal_relay(oracle_mod, alg, key_a, 0x77, 3 + i, inner)
        arena[i * SL:i * SL + len(pkt)] = list(pkt)
        packets.append((i * SL, len(pkt), 0))
        routes.append((0, 0xABC0 + i))
    res = M.forward(oracle_mod, R, alg, [key_a], arena, packets, routes, [(40, key_b)], 64)
    return R, key_a, key_b, inners, arena, packets, res


def test_model_forwarded_packet_opens_under_target_key(oracle_mod):
    for alg in (L.ALG_AESGCM, L.ALG_CHACHAPOLY):
        R, key_a, key_b, inners, arena, packets, (status, fwd, exp, wins, ctr) = _model_case(oracle_mod, alg)
        assert status == [R.OK] * 4 and fwd == [R.OK] * 4 and ctr == [44]
        for i, (off, ln, _) in enumerate(packets):
            out = bytes(exp[off:off + ln])
            c = 41 + i
            assert out[:16] == oracle_mod.header_encode(1, 1, 1, 0xABC0 + i, c)
            assert out[16:ln - 16] == inners[i] == bytes(arena[off + 16:off + ln - 16])  # inner bytes unchanged
            assert oracle_mod.open_(alg, key_b, oracle_mod.nonce(alg, c), out[:ln - 16], out[ln - 16:]) == b""
            for cc in (c, 3 + i):  # no longer under the inbound key, at either counter
                assert oracle_mod.open_(alg, key_a, oracle_mod.nonce(alg, cc), out[:ln - 16], out[ln - 16:]) is None
        assert wins[0].current == 6


def test_model_forgery_and_replay_take_no_counter(oracle_mod):
    import replay_oracle as R

    alg = L.ALG_AESGCM
    key_a, key_b = bytes(range(32)), bytes(range(1, 33))
    pk = [M.seal_relay(oracle_mod, alg, key_a, 1, 3 + i, b"x" * 9) for i in range(5)]
    bad = bytearray(pk[1])
    bad[20] ^= 1
    pk[1], pk[3] = bytes(bad), pk[0]
    SL = 64
    arena = np.zeros(SL * 5, np.uint8)
    for i, p in enumerate(pk):
        arena[i * SL:i * SL + len(p)] = list(p)
    packets = [(i * SL, len(p), 0) for i, p in enumerate(pk)]
    status, fwd, exp, _, ctr = M.forward(oracle_mod, R, alg, [key_a], arena, packets, [(0, 5)] * 5,
                                         [(M.REJECT_AFTER - 3, key_b)], 64)
    assert status == [R.OK, R.AUTH_FAILED, R.OK, R.REPLAY, R.OK]
    # counters REJECT_AFTER-2, -1, then REJECT_AFTER itself: exhausted, untouched, the counter used
    assert fwd == [R.OK, M.NOT_FORWARDED, R.OK, M.NOT_FORWARDED, R.EXHAUSTED] and ctr == [M.REJECT_AFTER]
    for i in (1, 3, 4):
        assert np.array_equal(exp[i * SL:(i + 1) * SL], arena[i * SL:(i + 1) * SL])
