"""GPU: neb_rx_open_via_batch[_host] — a receive batch of a node behind relays: VerifyRelay on the
outer packet, the unwrap, and the receive of the inner packet, in one call — against the deferred
sequential model in tests/rx_via_ref.py: statuses, inner records, the whole arena, and every
window's bits, current counter and statistics."""
import random

import numpy as np
import pytest

import rx_via_ref as M
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

ALGS = [L.ALG_AESGCM, L.ALG_CHACHAPOLY]
T = M.VIA_TERMINAL
NR = M.NOT_RELAYED


def _key(rng):
    return bytes(rng.getrandbits(8) for _ in range(32))


class _Node:
    """keys {tunnel: key | M.OTHER_ALG} installed on the engine (OTHER_ALG: a key of the other
    cipher in that tunnel's slot); the windows of one run or of several consecutive ones."""

    def __init__(self, engine, alg, keys, seed=0):
        from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

        cf, other = (CipherAESGCM, CipherChaChaPoly) if alg == L.ALG_AESGCM else (CipherChaChaPoly, CipherAESGCM)
        rng = random.Random(seed)
        self.engine, self.alg = engine, alg
        self.c = {t: (other.Cipher(engine, _key(rng)) if k == M.OTHER_ALG else cf.Cipher(engine, k)) for t, k in keys.items()}
        self.count = max(c.key_id for c in self.c.values()) + 1
        self.host, self.dw = None, None

    def key_id(self, t):
        return L.KEYS_MIXED if t is None else self.c[t].key_id

    def open_windows(self, device, window_len):
        from nebula_amd.connection_state import Bits, DeviceWindows

        self.host = {t: Bits(window_len) for t in self.c}
        if device:
            self.dw = DeviceWindows(self.engine, self.count, window_len)
            for t, c in self.c.items():
                self.dw.load(c.key_id, self.host[t])

    def close(self):
        if self.dw is not None:
            self.dw.destroy()
        for w in (self.host or {}).values():
            w.destroy()
        for c in self.c.values():
            c.destroy()

    def run(self, packets, via, arena, hints=(L.KEYS_MIXED, L.KEYS_MIXED), strict=False):
        """-> status, inner records, inner_status, arena; self.host holds the windows afterwards"""
        from nebula_amd.relay import rx_open_via_batch, rx_open_via_batch_device

        e, alg = self.engine, self.alg
        pk = np.array([(off, ln, self.key_id(t)) for off, ln, t in packets], dtype=L.RX_PACKET_DTYPE)
        vi = np.array([(self.key_id(g), fl) for g, fl in via], dtype=L.RX_VIA_DTYPE)
        arena = arena.copy()
        if self.dw is None:
            windows = [None] * self.count
            for t, c in self.c.items():
                windows[c.key_id] = self.host[t]
            st, inner, ist = rx_open_via_batch(e, alg, windows, pk, vi, arena, *hints)
            return st, inner, ist, arena
        import torch

        dev = torch.device("cuda", e.device)
        up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)  # noqa: E731
        n = len(pk)
        d_pk, d_vi, d_arena = up(pk), up(vi), up(arena)
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_ist = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_inner = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
        with L.knob(L.KNOB_RX_STRICT, 1 if strict else 0):
            rx_open_via_batch_device(e, alg, self.dw, d_pk, d_vi, d_arena, d_st, d_inner, d_ist, *hints)
        torch.cuda.synchronize()
        for t, c in self.c.items():
            self.dw.store(c.key_id, self.host[t])
        return (d_st.cpu().numpy(), d_inner.cpu().numpy().view(L.RX_PACKET_DTYPE).copy(), d_ist.cpu().numpy(),
                d_arena.cpu().numpy())


def _check(oracle_mod, node, owins, pkts, via, keys, slot, hints=(L.KEYS_MIXED, L.KEYS_MIXED), strict=False):
    """One call against the deferred model, which moves owins ({tunnel: replay_oracle.Bits}) on."""
    import replay_oracle as R

    arena, packets = M.lay_out(pkts, slot)
    exp_st, exp_inner, exp_ist, exp_arena = M.rx_via_deferred(oracle_mod, R, node.alg, keys, owins, arena, packets, via)
    st, inner, ist, got = node.run(packets, via, arena, hints, strict)
    assert st.tolist() == exp_st
    assert ist.tolist() == exp_ist
    assert [(int(r["off"]), int(r["len"]), int(r["key_id"])) for r in inner] == \
        [(off, ln, node.key_id(g)) for off, ln, g in exp_inner]
    bad = np.flatnonzero(got != exp_arena)
    assert bad.size == 0, f"first differing arena byte {bad[:4]} (slot {bad[0] // slot}, +{bad[0] % slot})"
    for t, o in owins.items():
        w = node.host[t]
        assert (w.current, w.lost, w.dupe, w.out_of_window) == (o.current, o.lost, o.dupe, o.out_of_window), t
        assert w.snapshot() == o.snapshot(), t
    return exp_st, exp_ist, got, packets, arena


def _one(engine, oracle_mod, alg, device, keys, pkts, via, window_len=64, slot=192, **kw):
    import replay_oracle as R

    node = _Node(engine, alg, keys)
    try:
        node.open_windows(device, window_len)
        owins = {t: R.Bits(window_len) for t in keys}
        return _check(oracle_mod, node, owins, pkts, via, keys, slot, **kw) + (owins,)
    finally:
        node.close()


@pytest.mark.parametrize("mode", ["none", "all", "third"])
@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_sizes_and_terminal_shares(engine, oracle_mod, n, mode):
    """The fused kernel's wave and workgroup edges. No terminal packet: phase 2 does not run; all:
    every packet runs both phases; every third, with forgeries, replays and short packets mixed in.
    The clean none / all batches must run the parallel form (NEB_RXDEV_STRICT refuses the host finish)."""
    alg = ALGS[(n + len(mode)) % 2]
    rng = random.Random(n * 7 + len(mode))
    keys, pkts, via = M.random_batch(oracle_mod, alg, rng, n, nrelay=2, ndirect=2, ntarget=3, noise=mode == "third")
    flag = {"none": lambda i: 0, "all": lambda i: T, "third": lambda i: T if i % 3 == 0 else 0}[mode]
    via = [(g, flag(i)) for i, (g, _) in enumerate(via)]
    st, ist, _, _, _, _ = _one(engine, oracle_mod, alg, True, keys, pkts, via, 1024, strict=mode != "third")
    if mode == "none":
        assert ist == [NR] * n
    if mode == "all":
        assert st == [0] * n and ist == [0] * n
    if mode == "third" and n >= 255:
        assert {0, 1, 5, NR} <= set(ist) and {0, 1, 4} <= set(st)


def _relay(oracle_mod, alg, keys, c, inner, t=0):
    return M.seal_relay(oracle_mod, alg, keys[t], 0x100 + t, c, inner)


def _msg(oracle_mod, alg, keys, t, c, pt=b"payload bytes", typ=1, sub=0):
    return M.seal_message(oracle_mod, alg, keys[t], 0x100 + t, c, pt, typ, sub)


def _flip(p, at):
    p = bytearray(p)
    p[at] ^= 0x10
    return bytes(p)


# Directed batches. Tunnel 0 is a relay, 1 and 2 are peers. Each entry builds
# ([(bytes, outer tunnel)], via, expected status, expected inner_status).
def _case_outer_forgery(om, alg, keys):
    p = _relay(om, alg, keys, 1, _msg(om, alg, keys, 1, 1))
    return [(_flip(p, 20), 0), (_flip(p, len(p) - 1), 0)], [(1, T)] * 2, [1, 1], [NR, NR]


def _case_outer_duplicate(om, alg, keys):
    p = _relay(om, alg, keys, 1, _msg(om, alg, keys, 1, 1))
    return [(p, 0), (p, 0)], [(1, T)] * 2, [0, 4], [0, NR]


def _case_forged_inner(om, alg, keys):
    p = _relay(om, alg, keys, 1, _flip(_msg(om, alg, keys, 1, 1), 20))
    q = _relay(om, alg, keys, 2, _flip(_msg(om, alg, keys, 1, 2), 16 + 13 + 15))  # the inner tag's last byte
    return [(p, 0), (q, 0)], [(1, T)] * 2, [0, 0], [1, 1]


def _case_inner_wrapped_twice(om, alg, keys):
    inner = _msg(om, alg, keys, 1, 7)
    return [(_relay(om, alg, keys, 1, inner), 0), (_relay(om, alg, keys, 2, inner), 0)], [(1, T)] * 2, [0, 0], [0, 4]


def _case_not_terminal(om, alg, keys):
    p = _relay(om, alg, keys, 1, _msg(om, alg, keys, 1, 1))
    return [(p, 0)], [(1, 0)], [0], [NR]


def _case_terminal_on_a_message(om, alg, keys):
    return [(_msg(om, alg, keys, 1, 1, bytes(60)), 1), (_msg(om, alg, keys, 2, 1, bytes(60), 4, 1), 2)], [(2, T), (1, T)], \
        [0, 0], [NR, NR]


def _case_nested_relay(om, alg, keys):
    inner = M.seal_relay(om, alg, keys[1], 0x101, 1, _msg(om, alg, keys, 2, 1))
    return [(_relay(om, alg, keys, 1, inner), 0), (_relay(om, alg, keys, 2, inner[:20]), 0)], [(1, T), (None, T)], \
        [0, 0], [7, 7]


def _case_inner_handshake(om, alg, keys):
    hs, rerr = om.header_encode(1, 0, 0, 9, 1) + bytes(50), om.header_encode(1, 2, 0, 9, 1)
    return [(_relay(om, alg, keys, 1, hs), 0), (_relay(om, alg, keys, 2, rerr), 0)], [(1, T), (None, T)], [0, 0], [7, 7]


def _case_inner_short(om, alg, keys):
    h = om.header_encode(1, 1, 0, 0x101, 1)
    inners = [b"", h[:1], h[:15], h + bytes(15)]  # outer lengths 32, 33, 47, 63
    pk = [(_relay(om, alg, keys, 1 + i, x), 0) for i, x in enumerate(inners)]
    assert [len(p) for p, _ in pk] == [32, 33, 47, 63]
    return pk, [(1, T)] * 4, [0] * 4, [5] * 4


def _case_inner_bad_key(om, alg, keys):
    return [(_relay(om, alg, keys, 1, _msg(om, alg, keys, 1, 1)), 0)], [(None, T)], [0], [3]


def _case_inner_key_of_the_other_cipher(om, alg, keys):
    keys[2] = M.OTHER_ALG
    inner = om.header_encode(1, 1, 0, 0x102, 1) + bytes(40)
    return [(_relay(om, alg, keys, 1, inner), 0), (_relay(om, alg, keys, 2, _msg(om, alg, keys, 1, 1)), 0)], \
        [(2, T), (1, T)], [0, 0], [3, 0]


def _case_direct_and_relayed_on_one_tunnel(om, alg, keys):
    # window 64: the direct counter is more than a window ahead of the relayed one, which arrives first
    return [(_relay(om, alg, keys, 1, _msg(om, alg, keys, 1, 5)), 0), (_msg(om, alg, keys, 1, 5 + 64 + 10), 1),
            (_relay(om, alg, keys, 2, _msg(om, alg, keys, 1, 5 + 64 + 9)), 0)], [(1, T), (None, 0), (1, T)], [0, 0, 0], [4, NR, 0]


CASES = {f.__name__[6:]: f for f in (
    _case_outer_forgery, _case_outer_duplicate, _case_forged_inner, _case_inner_wrapped_twice, _case_not_terminal,
    _case_terminal_on_a_message, _case_nested_relay, _case_inner_handshake, _case_inner_short, _case_inner_bad_key,
    _case_inner_key_of_the_other_cipher, _case_direct_and_relayed_on_one_tunnel)}


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_directed(engine, oracle_mod, case, alg, device):
    rng = random.Random(len(case))
    keys = {t: _key(rng) for t in range(3)}
    pkts, via, want_st, want_ist = CASES[case](oracle_mod, alg, keys)
    st, ist, got, packets, arena, owins = _one(engine, oracle_mod, alg, device, keys, pkts, via, 64, 128)
    assert st == want_st and ist == want_ist
    if case in ("outer_forgery", "not_terminal", "nested_relay", "inner_handshake", "inner_short", "inner_bad_key"):
        assert np.array_equal(got, arena)  # nothing written
        assert all(owins[t].current == 0 for t in (1, 2))  # and no inner window event
    if case == "outer_duplicate":
        assert (owins[1].current, owins[1].dupe) == (1, 0) and owins[0].dupe == 0  # Check refused the second: no Update
    if case == "forged_inner":
        assert (owins[0].current, owins[1].current) == (2, 0)
        for off, ln, _ in packets:
            assert not got[off + 32:off + ln - 32].any()  # the inner payload zeroed
            keep = np.r_[off:off + 32, off + ln - 32:off + ln]  # both headers, the inner tag, the outer tag
            assert np.array_equal(got[keep], arena[keep])
    if case == "inner_key_of_the_other_cipher":
        assert owins[2].current == 0 and np.array_equal(got[:128], arena[:128])


@pytest.mark.parametrize("alg", ALGS)
def test_many_target_windows(engine, oracle_mod, alg):
    """2 relay windows and 300 target windows (window indices past 8 bits: the inner sort's two passes)."""
    rng = random.Random(300 + alg)
    keys, pkts, via = M.random_batch(oracle_mod, alg, rng, 700, nrelay=2, ndirect=0, ntarget=300, payloads=(0, 20))
    st, ist, *_ = _one(engine, oracle_mod, alg, True, keys, pkts, via, 256, 128)
    assert ist.count(0) > 300 and {1, 4} <= set(ist)


@pytest.mark.parametrize("hints", [False, True])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("alg", ALGS)
def test_one_window_per_phase(engine, oracle_mod, alg, device, hints):
    """One relay and one peer behind it (the receive's no-sort path in both phases), with and
    without the two single-key hints."""
    import replay_oracle as R

    rng = random.Random(17 + alg)
    keys, pkts, via = M.random_batch(oracle_mod, alg, rng, 300 if device else 64, nrelay=1, ndirect=0, ntarget=1,
                                     terminal=1.0, noise=False)
    node = _Node(engine, alg, keys)
    try:
        node.open_windows(device, 512)
        owins = {t: R.Bits(512) for t in keys}
        h = (node.key_id(0), node.key_id(1)) if hints else (L.KEYS_MIXED, L.KEYS_MIXED)
        st, ist, *_ = _check(oracle_mod, node, owins, pkts, via, keys, 192, hints=h, strict=device)
        assert st == [0] * len(pkts) and ist == [0] * len(pkts)
    finally:
        node.close()


@pytest.mark.parametrize("device", [False, True])
def test_two_calls_continue_the_windows(engine, oracle_mod, device):
    """The second call sees the first one's windows: a datagram of the first batch again (outer
    REPLAY), and an inner packet of the first batch under a fresh outer counter (inner REPLAY)."""
    import replay_oracle as R

    alg = L.ALG_AESGCM
    rng = random.Random(23)
    keys = {t: _key(rng) for t in range(3)}
    inner = [_msg(oracle_mod, alg, keys, 1 + i % 2, 1 + i // 2, bytes([i]) * 30) for i in range(12)]
    first = [(_relay(oracle_mod, alg, keys, 1 + i, x), 0) for i, x in enumerate(inner[:8])]
    second = [first[2], (_relay(oracle_mod, alg, keys, 9, inner[3]), 0)] + \
        [(_relay(oracle_mod, alg, keys, 10 + i, x), 0) for i, x in enumerate(inner[8:])]
    node = _Node(engine, alg, keys)
    try:
        node.open_windows(device, 64)
        owins = {t: R.Bits(64) for t in keys}
        st1, ist1, *_ = _check(oracle_mod, node, owins, first, [(1 + i % 2, T) for i in range(8)], keys, 128)
        assert st1 == [0] * 8 and ist1 == [0] * 8
        via2 = [(1, T), (2, T)] + [(1 + i % 2, T) for i in range(4)]
        st2, ist2, *_ = _check(oracle_mod, node, owins, second, via2, keys, 128)
        assert st2 == [4, 0, 0, 0, 0, 0] and ist2 == [NR, 4, 0, 0, 0, 0]
        assert owins[0].current == 13 and owins[0].dupe == 0
    finally:
        node.close()


def test_relayed_tcp_flow_to_tun_writes(engine, oracle_mod):
    """inner_pk and inner_status go unchanged into neb_rx_plain_from_wire and neb_rx_coalesce_batch:
    a 40-segment TCP flow received through a relay, a relayed packet that fails its inner tag and a
    direct message in between, coalesces as the model says."""
    import torch

    import coalesce_cases as K
    import coalesce_ref as CM
    from nebula_amd import outside as O
    from nebula_amd.relay import rx_open_via_batch_device

    alg = L.ALG_AESGCM
    rng = random.Random(40)
    keys = {t: _key(rng) for t in range(3)}  # 0: the relay, 1: the peer behind it, 2: a direct peer
    node = _Node(engine, alg, keys)
    try:
        node.open_windows(True, 1024)
        pkts, via, expect = [], [], []
        for i in range(40):
            seg = K.seg(i, size=200)
            inner = _msg(oracle_mod, alg, keys, 1, 1 + i, seg)
            forged = i == 17
            pkts.append((_relay(oracle_mod, alg, keys, 1 + i, _flip(inner, 40) if forged else inner), 0))
            via.append((1, T))
            expect.append(dict(data=b"" if forged else seg, epoch=77, counter=1 + i, flags=CM.PLAIN_SKIP if forged else 0))
            if i == 20:
                pkts.append((_msg(oracle_mod, alg, keys, 2, 1, K.seg(0, size=100, sport=4000)), 2))
                via.append((None, 0))
                expect.append(dict(data=b"", epoch=0, counter=0, flags=CM.PLAIN_SKIP))
        n = len(pkts)
        arena, packets = M.lay_out(pkts, 320)
        pk = np.array([(off, ln, node.key_id(t)) for off, ln, t in packets], dtype=L.RX_PACKET_DTYPE)
        vi = np.array([(node.key_id(g), fl) for g, fl in via], dtype=L.RX_VIA_DTYPE)
        epoch = np.zeros(node.count, np.uint64)
        epoch[node.key_id(1)] = 77
        dev = torch.device("cuda", engine.device)
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_pk, d_vi, d_arena, d_epoch = up(pk), up(vi), up(arena), up(epoch)
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_ist = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_inner = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        cap = sum(CM.align16(len(p["data"])) for p in expect)
        d_plain = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
        d_writes = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_nw = torch.zeros(1, dtype=torch.int32, device=dev)
        d_pw = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ps = torch.zeros(n, dtype=torch.int32, device=dev)
        rx_open_via_batch_device(engine, alg, node.dw, d_pk, d_vi, d_arena, d_st, d_inner, d_ist)
        O.plain_from_wire_device(engine, d_inner, d_ist, d_epoch.view(torch.int64), d_arena, d_plain)
        O.coalesce_batch_device(engine, d_plain, d_arena, d_out[:cap], d_writes, d_nw, d_pw, d_ps)
        torch.cuda.synchronize(dev)
        assert (d_st.cpu().numpy() == 0).all()
        ist = d_ist.cpu().numpy().tolist()
        assert ist.count(0) == 39 and ist.count(1) == 1 and ist.count(NR) == 1
        model = CM.coalesce(expect, K.BOTH, cap, n)
        writes = d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:int(d_nw.item())]
        K.assert_equal_model(model, (writes, d_out.cpu().numpy(), d_pw.cpu().numpy().view(np.uint32), d_ps.cpu().numpy()),
                             "through a relay")
        assert max(w["nseg"] for w in model[0]) >= 17
    finally:
        node.close()


def test_argument_checks(engine):
    """Null pointers and n == 0, as the neighbouring calls."""
    import ctypes as C

    from nebula_amd.connection_state import DeviceWindows

    lib, e = L.lib(), engine
    dw = DeviceWindows(e, 4, 64)
    try:
        one = C.c_void_p(16)
        assert lib.neb_rx_open_via_batch(e.handle, L.ALG_AESGCM, dw.handle, None, None, 0, None, None, None, None,
                                         L.KEYS_MIXED, L.KEYS_MIXED, None) == L.OK
        assert lib.neb_rx_open_via_batch(e.handle, L.ALG_AESGCM, dw.handle, one, None, 1, one, one, one, one,
                                         L.KEYS_MIXED, L.KEYS_MIXED, None) == L.ERR_INVALID
        assert lib.neb_rx_open_via_batch(e.handle, L.ALG_AESGCM, None, one, one, 1, one, one, one, one, L.KEYS_MIXED,
                                         L.KEYS_MIXED, None) == L.ERR_INVALID
        assert lib.neb_rx_open_via_batch(e.handle, 99, dw.handle, one, one, 1, one, one, one, one, L.KEYS_MIXED,
                                         L.KEYS_MIXED, None) != L.OK
        assert lib.neb_rx_open_via_batch_host(e.handle, L.ALG_AESGCM, None, 0, None, None, 0, None, 0, None, None, None,
                                              L.KEYS_MIXED, L.KEYS_MIXED) == L.OK
        assert lib.neb_rx_open_via_batch_host(e.handle, L.ALG_AESGCM, None, 0, one, None, 1, one, 64, one, one, one,
                                              L.KEYS_MIXED, L.KEYS_MIXED) == L.ERR_INVALID
    finally:
        dw.destroy()
