"""CPU: the directed Poly1305 edge vectors (tests/poly1305_ref.py, tests/golden/poly1305_edges.json).

Three independent implementations — the Python-integer helper that solved the packets, the plain-C
oracle and OpenSSL EVP — give the same sealed bytes for every vector, the helper reproduces
RFC 8439 §2.8.2, every vector's accumulator is the value its name says, and the committed file is
what make_golden.py writes today. The GPU side (tests/test_gpu_auth_edges.py) then compares the
kernels with the committed bytes."""
import json
import os

import numpy as np
import pytest

import poly1305_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def committed():
    with open(os.path.join(GOLD, "poly1305_edges.json")) as f:
        return json.load(f)


def test_helper_reproduces_rfc8439():
    with open(os.path.join(GOLD, "kat.json")) as f:
        k = json.load(f)["chachapoly_rfc8439_2_8_2"]
    out = R.seal_nonce(bytes.fromhex(k["key"]), bytes.fromhex(k["iv"]), bytes.fromhex(k["aad"]),
                       bytes.fromhex(k["plaintext"]))
    assert out[-16:].hex() == k["expected_tag"]
    assert out[:16].hex() == k["expected_ct_prefix"]
    # RFC 8439 §2.5.2, Poly1305 alone
    key = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    r = int.from_bytes(key[:16], "little") & R.CLAMP
    s = int.from_bytes(key[16:], "little")
    assert R.tag_of(R.accumulate(r, b"Cryptographic Forum Research Group"), s).hex() == \
        "a8061dc1305136c6c22b8baf0c0127a9"


def test_every_target_in_both_shapes():
    """34 vectors: the 16 targets in the relay and the data shape, none skipped, both keys in
    each shape, and the all-0xFF packet of each shape."""
    vs = committed()
    assert len(vs) == 34
    assert [(v["shape"], v["target"]) for v in vs[:32]] == [(s, t) for s in R.SHAPES for t in R.EDGE_TARGETS]
    assert [(v["shape"], v["target"]) for v in vs[32:]] == [("relay", "all_ff"), ("data", "all_ff")]
    for shape in R.SHAPES:
        assert {v["key"] for v in vs if v["shape"] == shape} == {k.hex() for k in R.KEYS}
    for v in vs:
        aad, pt = bytes.fromhex(v["aad"]), bytes.fromhex(v["plaintext"])
        assert 1 <= v["counter"] <= R.MAX_COUNTER
        if v["target"] == "all_ff":
            assert (len(aad), len(pt)) == ((640, 0) if v["shape"] == "relay" else (16, 640))
        else:
            assert (len(aad), len(pt)) == ((48, 0) if v["shape"] == "relay" else (16, 48))


def test_regenerated_file_is_the_committed_one(oracle_mod):
    import make_golden

    with open(os.path.join(GOLD, "poly1305_edges.json")) as f:
        assert f.read() == make_golden.poly1305_edges_json()


def test_accumulator_equals_target():
    for v in committed():
        key, aad, pt = (bytes.fromhex(v[k]) for k in ("key", "aad", "plaintext"))
        h = R.accumulator(key, v["counter"], aad, pt)
        if v["target"] == "all_ff":
            ct = bytes.fromhex(v["sealed"])[:-16]
            assert set(aad) == {0xFF} and set(ct) <= {0xFF}
            continue
        t = R.target_value(v["target"], key, v["counter"])
        assert t is not None and h == t, (v["shape"], v["target"])
        _, s = R.one_time_key(key, R.nebula_nonce(v["counter"]))
        tag = bytes.fromhex(v["sealed"])[-16:]
        if v["target"] == "tag_zero_carry_every_word":
            assert tag == bytes(16) and all((h >> 32 * i & 0xFFFFFFFF) + (s >> 32 * i & 0xFFFFFFFF) >= 0xFFFFFFFF
                                            for i in range(4)) and (h + s) >> 128 == 1
        if v["target"] == "carry_out_of_word0_only":
            assert tag[:4] == bytes(4) and (h + s) >> 128 == 0 and h >> 32 == 0
            assert (s >> 32 & 0xFFFFFFFF) != 0xFFFFFFFF  # the carry stops in word 1


def test_helper_oracle_and_evp_agree(oracle_mod):
    for v in committed():
        key, aad, pt = (bytes.fromhex(v[k]) for k in ("key", "aad", "plaintext"))
        sealed = bytes.fromhex(v["sealed"])
        assert R.seal(key, v["counter"], aad, pt) == sealed, (v["shape"], v["target"])
        nonce = oracle_mod.nonce(oracle_mod.CHACHA, v["counter"])
        assert nonce == R.nebula_nonce(v["counter"])
        assert oracle_mod.seal(oracle_mod.CHACHA, key, nonce, aad, pt) == sealed
        assert oracle_mod.open_(oracle_mod.CHACHA, key, nonce, aad, sealed) == pt
        src = (len(aad) + 15) // 16 * 16
        arena = np.zeros(src + len(pt) + 16, np.uint8)
        arena[:len(aad)] = np.frombuffer(aad, np.uint8)
        arena[src:src + len(pt)] = np.frombuffer(pt, np.uint8)
        d = np.zeros(1, oracle_mod.DESC_DTYPE)
        d[0] = (src, src, 0, v["counter"], len(pt), len(aad), 0, 0)
        _, st = oracle_mod.evp_batch(oracle_mod.CHACHA, 0, np.frombuffer(key, np.uint8).copy(), d, arena)
        assert st[0] == 0 and arena[src:].tobytes() == sealed
        _, st = oracle_mod.evp_batch(oracle_mod.CHACHA, 1, np.frombuffer(key, np.uint8).copy(), d, arena)
        assert st[0] == 0 and arena[src:src + len(pt)].tobytes() == pt


def test_solve_reports_an_unreachable_target():
    """solve() returns None instead of a wrong packet (a target function that never applies)."""
    assert R.solve(R.KEYS[0], lambda r, s: None, "relay") is None
