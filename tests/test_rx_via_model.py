"""CPU: the receive through relays (neb_rx_open_via_batch[_host], include/nebula_aead.h) as a
model. tests/rx_via_ref.py states the batch's contract (rx_via_deferred) and the reference's
per-packet recursion (rx_via_strict): they agree whenever no tunnel takes a window event in both
phases of a batch, and differ in the one documented way where a tunnel does. The unwrap rule of
the library (neb_rx_via_unwrap_host, pure CPU) is checked against the model's."""
import os
import random
import re

import numpy as np
import pytest

import rx_via_ref as M
from nebula_amd import _lib as L

ALGS = [L.ALG_AESGCM, L.ALG_CHACHAPOLY]
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nebula_aead.h")


def test_rx_via_symbols_constants_and_layout():
    lib = L.lib()
    for s in ("neb_rx_open_via_batch", "neb_rx_open_via_batch_host", "neb_rx_via_unwrap_host"):
        assert hasattr(lib, s) and s in L.SIGNATURES, s
    text = open(HDR).read()
    val = lambda name: int(re.search(rf"#define {name} (\w+)", text).group(1), 0)  # noqa: E731
    assert val("NEB_VIA_TERMINAL") == L.VIA_TERMINAL == M.VIA_TERMINAL == 1
    assert val("NEB_STATUS_NOT_RELAYED") == L.STATUS_NOT_RELAYED == M.NOT_RELAYED == 9
    assert val("NEB_STATUS_NOT_MESSAGE") == L.STATUS_NOT_MESSAGE
    assert L.RX_VIA_DTYPE.itemsize == 8 and L.RX_VIA_DTYPE.names == ("key_id", "flags")
    struct = re.search(r"typedef struct neb_rx_via \{(.*?)\} neb_rx_via;", text, re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", struct) == ["key_id", "flags"]


def _both(oracle_mod, alg, keys, pkts, via, window_len, slot=192):
    import replay_oracle as R

    arena, packets = M.lay_out(pkts, slot)
    out = []
    for fn in (M.rx_via_deferred, M.rx_via_strict):
        wins = {t: R.Bits(window_len) for t in keys}
        res = fn(oracle_mod, R, alg, keys, wins, arena, packets, via)
        out.append((res, wins))
    return out, packets


@pytest.mark.parametrize("alg", ALGS)
def test_models_agree_when_the_phases_share_no_tunnel(oracle_mod, alg):
    """150 seeded batches per cipher: n <= 64, window lengths 1..1024, forged, replayed, re-wrapped
    and short packets mixed in. The generator keeps the tunnels of the two phases apart; that is
    asserted per batch, so a generator bug cannot hide a case."""
    seen_inner, seen_outer = set(), set()
    for seed in range(150):
        rng = random.Random(1000 * alg + seed)
        n = rng.choice([1, 2, 7, 33, 64])
        wl = 1 << rng.randrange(11)
        keys, pkts, via = M.random_batch(oracle_mod, alg, rng, n, nrelay=rng.choice([1, 2]), ndirect=rng.choice([0, 2]),
                                         ntarget=rng.choice([1, 3]))
        phase1 = {t for _, t in pkts if t is not None}
        phase2 = {g for g, fl in via if g is not None and fl & M.VIA_TERMINAL}
        assert not (phase1 & phase2), (seed, phase1, phase2)
        ((d, dw), (s, sw)), _ = _both(oracle_mod, alg, keys, pkts, via, wl)
        assert d[0] == s[0] and d[1] == s[1] and d[2] == s[2], seed
        assert np.array_equal(d[3], s[3]), seed
        for t in keys:
            assert M.win_state(dw[t]) == M.win_state(sw[t]), (seed, t)
        seen_outer |= set(d[0])
        seen_inner |= set(d[2])
    assert {0, 1, 4, 5} <= seen_outer, seen_outer
    assert {0, 1, 3, 4, 5, 7, M.NOT_RELAYED} <= seen_inner, seen_inner


@pytest.mark.parametrize("alg", ALGS)
def test_shared_tunnel_is_the_strict_loop_with_direct_packets_first(oracle_mod, alg):
    """A peer T heard through a relay and then directly, the direct packet more than a window
    ahead. The strict loop accepts both (the relayed counter arrives first). The batch runs the
    direct packet first, so the relayed counter is out of the window: REPLAY. That outcome is the
    strict loop's for the arrival order with the direct packet first."""
    import replay_oracle as R

    rng = random.Random(alg)
    wl = 16
    keys = {t: bytes(rng.getrandbits(8) for _ in range(32)) for t in (0, 1)}  # 0: the relay, 1: T
    inner = M.seal_message(oracle_mod, alg, keys[1], 0x11, 5, b"through the relay")
    relayed = (M.seal_relay(oracle_mod, alg, keys[0], 0x10, 1, inner), 0)
    direct = (M.seal_message(oracle_mod, alg, keys[1], 0x11, 5 + wl + 10, b"direct"), 1)
    term, none = (1, M.VIA_TERMINAL), (None, 0)
    ((d, dw), (s, sw)), packets = _both(oracle_mod, alg, keys, [relayed, direct], [term, none], wl)
    assert s[0] == [0, 0] and s[2] == [0, M.NOT_RELAYED]
    assert d[0] == [0, 0] and d[2] == [R.REPLAY, M.NOT_RELAYED]
    assert sw[1].lost != dw[1].lost or sw[1].out_of_window != dw[1].out_of_window
    off = packets[0][0]
    assert bytes(s[3][off + 32:off + 32 + 17]) == b"through the relay"
    assert bytes(d[3][off:off + len(relayed[0])]) == relayed[0]  # refused by Check: not opened
    # the same two datagrams with the direct one first, through the strict loop
    ((_, _), (s2, s2w)), _ = _both(oracle_mod, alg, keys, [direct, relayed], [none, term], wl)
    assert s2[0] == [d[0][1], d[0][0]] and s2[2] == [d[2][1], d[2][0]]
    for t in keys:
        assert M.win_state(s2w[t]) == M.win_state(dw[t])


def _unwrap_cases(oracle_mod):
    """(bytes, status given, via key, flags): every reason a packet is not eligible, and len == 32."""
    relay = lambda inner: oracle_mod.header_encode(1, 1, 1, 5, 9) + inner + bytes(16)  # noqa: E731
    msg = oracle_mod.header_encode(1, 1, 0, 5, 9) + bytes(40)
    T = L.VIA_TERMINAL
    cases = [(relay(bytes(50)), 0, 7, T),            # eligible
             (relay(b""), 0, 7, T),                  # eligible, len == 32: an inner packet of 0 bytes
             (relay(b"x"), 0, L.KEYS_MIXED, T),      # eligible without an inner tunnel
             (relay(bytes(50)), 0, 7, T | 0x70),     # other flag bits are ignored
             (relay(bytes(50)), 0, 7, 0),            # not terminal
             (relay(bytes(50)), 0, 7, 2),            # not terminal (another bit)
             (msg, 0, 7, T),                         # not a relay packet
             (oracle_mod.header_encode(1, 4, 1, 5, 9) + bytes(40), 0, 7, T),  # subtype 1 of another type
             (oracle_mod.header_encode(1, 1, 1, 5, 9)[:12], L.STATUS_INVALID, 7, T)]
    cases += [(relay(bytes(50)), st, 7, T) for st in (1, 2, 3, 4, 5, 6, 7, 8, 9, -1)]  # the outer did not verify
    return cases


def test_unwrap_host_matches_the_model(oracle_mod):
    from nebula_amd.relay import rx_via_unwrap

    cases = _unwrap_cases(oracle_mod)
    arena, packets = M.lay_out([(c[0], None) for c in cases], 128)
    pk = np.array([(off, ln | (L.RX_OWN_SOURCE if i == 3 else 0), 0x55) for i, (off, ln, _) in enumerate(packets)],
                  dtype=L.RX_PACKET_DTYPE)
    via = np.array([(c[2], c[3]) for c in cases], dtype=L.RX_VIA_DTYPE)
    status = np.array([c[1] for c in cases], dtype=np.int32)
    before = arena.copy()
    inner, ist = rx_via_unwrap(pk, via, status, arena)
    assert np.array_equal(arena, before)
    eligible = 0
    for i, ((off, ln, _), c) in enumerate(zip(packets, cases)):
        key = None if c[2] == L.KEYS_MIXED else c[2]
        ok, (ioff, iln, ikey) = M.unwrap(c[1], c[0][:2], off, ln, (key, c[3]))
        assert (int(inner[i]["off"]), int(inner[i]["len"])) == (ioff, iln), i
        assert int(inner[i]["key_id"]) == (L.KEYS_MIXED if ikey is None else ikey), i
        assert ist[i] == (L.STATUS_OK if ok else L.STATUS_NOT_RELAYED), i
        assert not int(inner[i]["len"]) & L.RX_OWN_SOURCE
        eligible += ok
    assert eligible == 4 and int(inner[1]["len"]) == 0 and int(inner[1]["off"]) == packets[1][0] + 16


def test_unwrap_host_checks_records_against_the_arena(oracle_mod):
    lib = L.lib()
    arena = np.zeros(256, np.uint8)
    arena[:16] = np.frombuffer(oracle_mod.header_encode(1, 1, 1, 5, 9), np.uint8)
    vp = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)  # noqa: E731
    via = np.array([(7, L.VIA_TERMINAL)] * 2, dtype=L.RX_VIA_DTYPE)
    status = np.zeros(2, np.int32)
    for bad in ((200, 57), (257, 0), (2 ** 63, 64), (0, 0x7FFFFFFF)):
        pk = np.array([(0, 64, 1), (bad[0], bad[1], 1)], dtype=L.RX_PACKET_DTYPE)
        inner = np.full(2, 0xEE, np.uint8).repeat(16).view(L.RX_PACKET_DTYPE).copy()
        ist = np.full(2, -7, np.int32)
        keep = inner.copy()
        rc = lib.neb_rx_via_unwrap_host(vp(pk), vp(via), vp(status), 2, vp(arena), arena.nbytes, vp(inner), vp(ist))
        assert rc == L.ERR_INVALID, bad
        assert np.array_equal(inner, keep) and (ist == -7).all(), bad
    pk = np.array([(0, 64, 1), (192, 64, 1)], dtype=L.RX_PACKET_DTYPE)  # ends exactly at arena_len
    inner = np.zeros(2, L.RX_PACKET_DTYPE)
    ist = np.full(2, -7, np.int32)
    assert lib.neb_rx_via_unwrap_host(vp(pk), vp(via), vp(status), 2, vp(arena), arena.nbytes, vp(inner), vp(ist)) == L.OK
    assert ist.tolist() == [L.STATUS_OK, L.STATUS_NOT_RELAYED]
    assert lib.neb_rx_via_unwrap_host(None, None, None, 0, None, 0, None, None) == L.OK
    assert lib.neb_rx_via_unwrap_host(vp(pk), None, vp(status), 2, vp(arena), arena.nbytes, vp(inner), vp(ist)) == L.ERR_INVALID
