"""GPU: neb_relay_forward_batch[_host] — a relay node's receive batch with every verified
Message/Relay packet forwarded in place (VerifyRelay, then SendVia) — against the sequential model
in tests/relay_forward_ref.py, and against the engine's own receive and TX batch."""
import random

import numpy as np
import pytest

import relay_forward_ref as M
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

ALGS = [L.ALG_AESGCM, L.ALG_CHACHAPOLY]
# the smallest batch the one-workgroup plan does not take (relay.hpp kRelayPlanSmallMax = 1024 x 8)
RELAY_PLAN_SMALL_MAX = 8192


def _keys(rng, n):
    return [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(n)]


def _lay_out(pkts, slot):
    """pkts: [(bytes, inbound tunnel or None)] -> arena, [(off, len, tunnel)]"""
    arena = np.zeros(max(len(pkts), 1) * slot, np.uint8)
    packets = []
    for i, (p, t) in enumerate(pkts):
        arena[i * slot:i * slot + len(p)] = np.frombuffer(p, np.uint8)
        packets.append((i * slot, len(p), t))
    return arena, packets


class _Node:
    """Inbound keys and target tunnel keys installed on the engine; runs one forward batch."""

    def __init__(self, engine, alg, in_keys, tun_keys):
        from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

        cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
        self.engine, self.alg = engine, alg
        self.cin = [cf.Cipher(engine, k) for k in in_keys]
        self.cout = [cf.Cipher(engine, k) if k is not None else None for k in tun_keys]

    def close(self):
        for c in self.cin + self.cout:
            if c is not None:
                c.destroy()

    def rx_packets(self, packets):
        pk = np.zeros(len(packets), L.RX_PACKET_DTYPE)
        for i, (off, ln, t) in enumerate(packets):
            pk[i] = (off, ln, self.cin[t].key_id if t is not None else L.KEYS_MIXED)
        return pk

    def tunnels(self, counters, remote=0x5000):
        from nebula_amd.inside import TX_TUNNEL_DTYPE

        tun = np.zeros(len(self.cout), TX_TUNNEL_DTYPE)
        for i, c in enumerate(self.cout):
            tun[i] = (counters[i], c.key_id if c is not None else L.KEYS_MIXED, remote + i)
        return tun

    def windows(self, window_len, seen=(1, 2)):
        from nebula_amd.connection_state import Bits

        ws = []
        for _ in self.cin:
            w = Bits(window_len)
            for c in seen:
                w.Update(c)
            ws.append(w)
        return ws

    def run(self, device, packets, routes, tun, arena, window_len, key_hint=L.KEYS_MIXED, forward=True):
        """-> status, fwd_status (None for the plain receive), arena, windows, tunnels"""
        from nebula_amd.connection_state import DeviceWindows, rx_open_wire_batch, rx_open_wire_batch_device
        from nebula_amd.relay import relay_forward_batch, relay_forward_batch_device

        e, alg = self.engine, self.alg
        pk = self.rx_packets(packets)
        rt = np.array(routes, dtype=L.RELAY_ROUTE_DTYPE)
        ewins = self.windows(window_len)
        arena, tun = arena.copy(), tun.copy()
        if not device:
            windows = [None] * e.max_keys
            for c, w in zip(self.cin, ewins):
                windows[c.key_id] = w
            if forward:
                st, fwd = relay_forward_batch(e, alg, windows, pk, rt, tun, arena, key_hint)
            else:
                st, fwd = rx_open_wire_batch(e, alg, windows, pk, arena, key_hint), None
            return st, fwd, arena, ewins, tun
        import torch

        dev = torch.device("cuda", e.device)
        dw = DeviceWindows(e, e.max_keys, window_len)
        try:
            for c, w in zip(self.cin, ewins):
                dw.load(c.key_id, w)
            up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)  # noqa: E731
            d_pk, d_rt, d_tun, d_arena = up(pk), up(rt), up(tun), up(arena)
            d_st = torch.full((len(pk),), -1, dtype=torch.int32, device=dev)
            d_fwd = torch.full((len(pk),), -1, dtype=torch.int32, device=dev)
            if forward:
                relay_forward_batch_device(e, alg, dw, d_pk, d_rt, d_tun, d_arena, d_st, d_fwd, key_hint)
            else:
                rx_open_wire_batch_device(e, alg, dw, d_pk, d_arena, d_st, key_hint)
            torch.cuda.synchronize()
            for c, w in zip(self.cin, ewins):
                dw.store(c.key_id, w)
            from nebula_amd.inside import TX_TUNNEL_DTYPE

            return (d_st.cpu().numpy(), d_fwd.cpu().numpy() if forward else None, d_arena.cpu().numpy(), ewins,
                    d_tun.cpu().numpy().view(TX_TUNNEL_DTYPE).copy())
        finally:
            dw.destroy()


def _check_against_model(oracle_mod, node, device, in_keys, tun_keys, counters, pkts, routes, window_len, slot,
                         key_hint=L.KEYS_MIXED):
    import replay_oracle as R

    arena, packets = _lay_out(pkts, slot)
    exp = M.forward(oracle_mod, R, node.alg, in_keys, arena, packets, routes, list(zip(counters, tun_keys)),
                    window_len)
    exp_status, exp_fwd, exp_arena, owins, exp_ctr = exp
    st, fwd, got, ewins, tun = node.run(device, packets, routes, node.tunnels(counters), arena, window_len, key_hint)
    assert st.tolist() == exp_status
    assert fwd.tolist() == exp_fwd
    bad = np.flatnonzero(got != exp_arena)
    assert bad.size == 0, f"first differing arena byte {bad[:4]} (slot {bad[0] // slot}, +{bad[0] % slot})"
    for t, w in enumerate(ewins):
        o = owins[t]
        assert (w.current, w.lost, w.dupe, w.out_of_window) == (o.current, o.lost, o.dupe, o.out_of_window)
    assert [int(c) for c in tun["message_counter"]] == exp_ctr
    return exp_status, exp_fwd, got, packets


def _parity_batch(oracle_mod, alg, in_keys, seed):
    """~300 packets, shuffled: relay packets of every inner length over six routes (two share a target
    tunnel, one names a keyless tunnel, one an index out of range, one none), ordinary messages,
    forgeries, replays, runts, handshake and recv-error headers."""
    rng = random.Random(seed)
    routes_of = [(0, 0xA0), (0, 0xA1), (1, 0xB0), (2, 0xC0), (7, 0xD0), (M.RELAY_NONE, 0), (3, 0xE0)]
    ctr = {t: 2 for t in range(len(in_keys))}
    items, sent = [], []  # (bytes, inbound tunnel, route)
    inner_lens = [0, 1, 15, 16, 17, 100, 1300]
    for k in range(290):
        t = rng.randrange(len(in_keys))
        route = routes_of[k % len(routes_of)]
        r = rng.random()
        if r < 0.12 and sent:
            items.append(rng.choice(sent))  # a replay of an earlier packet
            continue
        ctr[t] += 1 + (rng.random() < 0.1) * rng.randrange(1, 20)
        if r < 0.75:
            inner = bytes(rng.getrandbits(8) for _ in range(inner_lens[(k + k // 7) % 7]))  # every length on every route
            pkt = bytearray(M.seal_relay(oracle_mod, alg, in_keys[t], 0x1000 + t, ctr[t], inner))
        else:
            pt = bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 20, 576])))
            pkt = bytearray(M.seal_message(oracle_mod, alg, in_keys[t], 0x1000 + t, ctr[t], pt))
        if rng.random() < 0.08:
            pkt[rng.randrange(16, len(pkt))] ^= 1 << rng.randrange(8)  # a forgery
        items.append((bytes(pkt), t, route))
        sent.append(items[-1])
    some = routes_of[0]
    items += [(bytes([0x10, 0, 0, 0]) + bytes(60), 0, some), (bytes([0x12, 0]) + bytes(40), 1, some)]  # handshake, recv error
    items += [(b"", 0, some), (b"\x11\x01", 0, some), (bytes([0x11, 1]) + bytes(29), 0, some)]         # runts
    items += [(M.seal_relay(oracle_mod, alg, in_keys[1], 9, 900, b"no tunnel"), None, some)]
    rng.shuffle(items)
    return [(p, t) for p, t, _ in items], [r for _, _, r in items]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("alg", ALGS)
def test_relay_forward_matches_sequential_model(engine, oracle_mod, alg, device):
    import replay_oracle as R

    rng = random.Random(11 * alg + device)
    in_keys, tun_keys = _keys(rng, 3), _keys(rng, 4)
    tun_keys[2] = None  # a target tunnel without a key
    pkts, routes = _parity_batch(oracle_mod, alg, in_keys, seed=alg + 2 * device)
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        st, fwd, _, _ = _check_against_model(oracle_mod, node, device, in_keys, tun_keys, [10, 2 ** 33, 5, 77], pkts,
                                             routes, 256, 1600)
        assert {R.OK, M.NOT_FORWARDED, R.BAD_KEY} <= set(fwd), set(fwd)
        assert {R.OK, R.INVALID, R.NOT_MESSAGE, R.BAD_KEY, R.REPLAY, R.AUTH_FAILED} <= set(st), set(st)
    finally:
        node.close()


def _five(oracle_mod, alg, key):
    """Five relay packets of one inbound tunnel; the 2nd forged, the 4th a replay of the 1st."""
    pk = [M.seal_relay(oracle_mod, alg, key, 1, 3 + i, bytes([i]) * (7 + i)) for i in range(5)]
    bad = bytearray(pk[1])
    bad[-1] ^= 0x80
    pk[1], pk[3] = bytes(bad), pk[0]
    return [(p, 0) for p in pk]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("alg", ALGS)
def test_relay_forward_counter_order(engine, oracle_mod, alg, device):
    rng = random.Random(5)
    in_keys, tun_keys = _keys(rng, 1), _keys(rng, 1)
    c = 1000
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        pkts = _five(oracle_mod, alg, in_keys[0])
        _, fwd, got, packets = _check_against_model(oracle_mod, node, device, in_keys, tun_keys, [c], pkts,
                                                    [(0, 0x42)] * 5, 64, 64)
        assert fwd == [0, M.NOT_FORWARDED, 0, M.NOT_FORWARDED, 0]
        heads = [bytes(got[off:off + 16]) for off, _, _ in packets]
        assert [heads[i] for i in (0, 2, 4)] == [oracle_mod.header_encode(1, 1, 1, 0x42, c + k) for k in (1, 2, 3)]
    finally:
        node.close()


@pytest.mark.parametrize("device", [False, True])
def test_relay_forward_exhaustion(engine, oracle_mod, device):
    """A tunnel at REJECT_AFTER - 3: counters REJECT_AFTER - 2 and - 1 forward, the other four are
    exhausted, untouched, and still use their counters, as segment_oracle.tx_batch gives a tunnel
    for six segments."""
    import segment_oracle as S

    alg = L.ALG_AESGCM
    rng = random.Random(6)
    in_keys, tun_keys = _keys(rng, 1), _keys(rng, 1)
    start = M.REJECT_AFTER - 3
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        pkts = [(M.seal_relay(oracle_mod, alg, in_keys[0], 1, 3 + i, b"y" * i), 0) for i in range(6)]
        _, fwd, got, packets = _check_against_model(oracle_mod, node, device, in_keys, tun_keys, [start], pkts,
                                                    [(0, 1)] * 6, 64, 64)
        # the TX batch's rule for six one-segment packets of that tunnel
        wires, _, ctr = S.tx_batch(alg, [dict(counter=start, remote_index=1, key=tun_keys[0])],
                                   [dict(data=b"z", tunnel=0, flags=0, gso_type=0, hdr_len=0, gso_size=0, csum_start=0,
                                         csum_offset=0)] * 6, 1 << 20, 64,
                                   lambda a, k, c, ad, pt: oracle_mod.seal(a, k, oracle_mod.nonce(a, c), ad, pt),
                                   oracle_mod.header_encode)
        assert fwd == [w[5] for w in wires] == [0, 0, 2, 2, 2, 2]
        assert ctr == [start + 6]
        for i, (off, ln, _) in enumerate(packets):
            if fwd[i] == L.STATUS_EXHAUSTED:
                assert bytes(got[off:off + ln]) == pkts[i][0]
    finally:
        node.close()


@pytest.mark.parametrize("alg", ALGS)
def test_relay_forward_chain(engine, oracle_mod, alg):
    """What the forward wrote verifies on the next hop: a second receive with the target keys and
    fresh windows accepts every forwarded packet (no model involved)."""
    rng = random.Random(7 + alg)
    in_keys, tun_keys = _keys(rng, 2), _keys(rng, 3)
    pkts, routes = [], []
    for i in range(96):
        t = i % 2
        inner = bytes(rng.getrandbits(8) for _ in range([0, 1, 15, 16, 17, 100, 1300][i % 7]))
        pkts.append((M.seal_relay(oracle_mod, alg, in_keys[t], t, 3 + i, inner), t))
        routes.append((i % 3, 0x900 + i % 3))
    arena, packets = _lay_out(pkts, 1400)
    hop1 = _Node(engine, alg, in_keys, tun_keys)
    hop2 = _Node(engine, alg, tun_keys, [])
    try:
        st, fwd, out, _, tun = hop1.run(True, packets, routes, hop1.tunnels([2, 2, 2]), arena, 256)
        assert (st == 0).all() and (fwd == 0).all()
        assert tun["message_counter"].tolist() == [34, 34, 34]
        nxt = [(off, ln, routes[i][0]) for i, (off, ln, _) in enumerate(packets)]
        st2, _, out2, wins, _ = hop2.run(True, nxt, routes, hop2.tunnels([]), out, 256, forward=False)
        assert (st2 == 0).all()
        assert np.array_equal(out2, out)  # VerifyRelay writes nothing
        assert [w.current for w in wins] == [34, 34, 34]
    finally:
        hop1.close()
        hop2.close()


def test_relay_forward_shares_counters_with_tx_batch(engine, oracle_mod):
    """neb_tx_seal_batch, a forward, neb_tx_seal_batch on one tunnel array and stream: each tunnel's
    counters are contiguous across the three and none repeats."""
    import torch

    from nebula_amd.connection_state import DeviceWindows
    from nebula_amd.inside import TX_PACKET_DTYPE, TX_TUNNEL_DTYPE, DeviceTxBatch
    from nebula_amd.relay import relay_forward_batch_device

    alg = L.ALG_AESGCM
    rng = random.Random(8)
    in_keys, tun_keys = _keys(rng, 1), _keys(rng, 2)
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        start = [100, 7000]
        tun = node.tunnels(start)
        ntx = 10
        txp = np.zeros(ntx, TX_PACKET_DTYPE)
        for i in range(ntx):
            txp[i] = (i * 64, 40 + i, i % 2, 0, 0, 0, 0, 0, 0, 0)
        tun_reads = np.frombuffer(bytes(rng.getrandbits(8) for _ in range(ntx * 64)), np.uint8)
        db = DeviceTxBatch(engine, alg, tun, txp, tun_reads, 1 << 16, 64)
        nfw = 9
        pkts = [(M.seal_relay(oracle_mod, alg, in_keys[0], 1, 3 + i, b"q" * i), 0) for i in range(nfw)]
        routes = [(0 if i % 3 else 1, 0x33) for i in range(nfw)]
        arena, packets = _lay_out(pkts, 64)
        dev = torch.device("cuda", engine.device)
        dw = DeviceWindows(engine, engine.max_keys, 64)
        try:
            dw.load(node.cin[0].key_id, node.windows(64)[0])
            up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)  # noqa: E731
            d_pk, d_rt, d_arena = up(node.rx_packets(packets)), up(np.array(routes, dtype=L.RELAY_ROUTE_DTYPE)), up(arena)
            d_st = torch.full((nfw,), -1, dtype=torch.int32, device=dev)
            d_fwd = torch.full((nfw,), -1, dtype=torch.int32, device=dev)
            db.seal()
            r1 = db.result()
            relay_forward_batch_device(engine, alg, dw, d_pk, d_rt, db.tunnels, d_arena, d_st, d_fwd)
            db.seal()
            torch.cuda.synchronize()
            r2 = db.result()
            out = d_arena.cpu().numpy()
            assert (d_fwd.cpu().numpy() == 0).all()
        finally:
            dw.destroy()
        used = {0: [], 1: []}
        for w in r1.wires:
            used[int(txp[int(w["packet"])]["tunnel"])].append(int(w["counter"]))
        for i, (off, _, _) in enumerate(packets):
            used[routes[i][0]].append(int.from_bytes(bytes(out[off + 8:off + 16]), "big"))
        for w in r2.wires:
            used[int(txp[int(w["packet"])]["tunnel"])].append(int(w["counter"]))
        for t in (0, 1):
            assert used[t] == list(range(start[t] + 1, start[t] + 1 + len(used[t]))), (t, used[t])
            assert int(r2.tunnels[t]["message_counter"]) == start[t] + len(used[t])
        assert len(used[0]) + len(used[1]) == 2 * ntx + nfw
        assert r2.tunnels.dtype == TX_TUNNEL_DTYPE
    finally:
        node.close()


@pytest.mark.parametrize("alg", ALGS)
def test_relay_forward_grid_wide_plan(engine, oracle_mod, alg):
    """One packet more than the one-workgroup plan takes: 64 target tunnels with uneven shares,
    inner lengths 0..64, 2% forgeries."""
    rng = random.Random(9 + alg)
    n = RELAY_PLAN_SMALL_MAX + 1
    in_keys, tun_keys = _keys(rng, 4), _keys(rng, 64)
    pkts, routes = [], []
    ctr = [2] * 4
    for i in range(n):
        t = rng.randrange(4)
        ctr[t] += 1
        pkt = bytearray(M.seal_relay(oracle_mod, alg, in_keys[t], t, ctr[t], bytes([i & 255]) * (i % 65)))
        if rng.random() < 0.02:
            pkt[rng.randrange(16, len(pkt))] ^= 4
        pkts.append((bytes(pkt), t))
        tt = min(int(rng.expovariate(0.12)), 63)  # uneven shares
        routes.append((tt, 0x700 + tt))
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        _, fwd, _, _ = _check_against_model(oracle_mod, node, True, in_keys, tun_keys, [1000 * t for t in range(64)],
                                            pkts, routes, 8192, 112)
        assert fwd.count(0) > 0.9 * n and M.NOT_FORWARDED in fwd
    finally:
        node.close()


@pytest.mark.parametrize("device", [False, True])
def test_relay_forward_leaves_the_receive_unchanged(engine, oracle_mod, device):
    """status, the bytes of every packet that is not forwarded and the windows equal the plain
    neb_rx_open_wire_batch[_host] on the same input."""
    alg = L.ALG_AESGCM
    rng = random.Random(10 + device)
    in_keys, tun_keys = _keys(rng, 3), _keys(rng, 4)
    tun_keys[2] = None
    pkts, routes = _parity_batch(oracle_mod, alg, in_keys, seed=40 + device)
    arena, packets = _lay_out(pkts, 1600)
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        tun = node.tunnels([1, 2, 3, 4])
        st, fwd, got, wins, _ = node.run(device, packets, routes, tun, arena, 256)
        st0, _, got0, wins0, _ = node.run(device, packets, routes, tun, arena, 256, forward=False)
        assert st.tolist() == st0.tolist()
        for i, (off, ln, _) in enumerate(packets):
            if fwd[i] != 0:
                assert np.array_equal(got[off:off + 1600], got0[off:off + 1600]), i
            else:  # forwarded: only the header and the tag may differ
                assert np.array_equal(got[off + 16:off + ln - 16], got0[off + 16:off + ln - 16]), i
                assert np.array_equal(got[off + ln:off + 1600], got0[off + ln:off + 1600]), i
        for w, w0 in zip(wins, wins0):
            assert (w.current, w.lost, w.dupe, w.out_of_window) == (w0.current, w0.lost, w0.dupe, w0.out_of_window)
        assert (fwd == 0).sum() > 50
    finally:
        node.close()


@pytest.mark.parametrize("n", [1025, 2049])
def test_relay_forward_one_workgroup_plan_sizes(engine, oracle_mod, n):
    """The one-workgroup plan past one packet per thread (the mark runs grid-wide first): 2 packets
    per thread up to 2048, 8 above."""
    alg = L.ALG_AESGCM
    rng = random.Random(n)
    in_keys, tun_keys = _keys(rng, 2), _keys(rng, 5)
    pkts, routes = [], []
    for i in range(n):
        t = i & 1
        pkt = bytearray(M.seal_relay(oracle_mod, alg, in_keys[t], t, 3 + i // 2, bytes([i & 255]) * (i % 19)))
        if rng.random() < 0.03:
            pkt[-1] ^= 1
        pkts.append((bytes(pkt), t))
        routes.append((rng.choice([0, 0, 0, 1, 2, 3, 4, 9, M.RELAY_NONE]), i))
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        _, fwd, _, _ = _check_against_model(oracle_mod, node, True, in_keys, tun_keys, [7, 0, 1 << 40, 3, 99], pkts,
                                            routes, 2048, 64)
        assert {0, 3, M.NOT_FORWARDED} <= set(fwd)
    finally:
        node.close()


@pytest.mark.parametrize("device", [False, True])
def test_relay_forward_nothing_to_forward(engine, oracle_mod, device):
    """No tunnels at all and no packet with a usable route: the receive still runs, nothing is written."""
    alg = L.ALG_CHACHAPOLY
    rng = random.Random(3)
    in_keys = _keys(rng, 1)
    pkts = [(M.seal_relay(oracle_mod, alg, in_keys[0], 1, 3 + i, b"k" * i), 0) for i in range(8)]
    routes = [(M.RELAY_NONE, 0)] * 4 + [(0, 1)] * 4
    node = _Node(engine, alg, in_keys, [])
    try:
        st, fwd, got, packets = _check_against_model(oracle_mod, node, device, in_keys, [], [], pkts, routes, 64, 64)
        assert st == [0] * 8 and fwd == [M.NOT_FORWARDED] * 4 + [3] * 4
        assert np.array_equal(got, _lay_out(pkts, 64)[0])
    finally:
        node.close()
