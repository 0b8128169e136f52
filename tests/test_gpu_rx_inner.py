"""GPU: neb_rx_inner_batch — newPacket(incoming) and firewall.Drop's two address checks for a whole
opened batch on the device — against the host form and the model (tests/rx_inner_ref.py) on the
cases of tests/rx_inner_cases.py, over several table states, and between a real receive's open and
its coalescer."""
import ctypes as C
import ipaddress
import random

import numpy as np
import pytest

import rx_inner_cases as RC
import rx_inner_ref as M
from nebula_amd import _lib as L
from nebula_amd import outside as O
from nebula_amd.hostmap import PeerTable, peer_nets, routable

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257)
PLAIN, FW = L.PLAIN_PACKET_DTYPE.itemsize, L.FW_PACKET_DTYPE.itemsize
EP = np.array(RC.EPOCHS, np.uint64)


def _dev(engine):
    import torch

    return torch.device("cuda", engine.device)


def _up(engine, a, skew=0):
    """The bytes of `a` on the device, `skew` bytes past an allocation's (256-byte aligned) base."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.empty(len(b) + skew, dtype=torch.uint8, device=_dev(engine))
    d[skew:] = torch.from_numpy(b.copy()).to(_dev(engine))
    return d[skew:]


def _outputs(engine, n):
    import torch

    return (torch.full((n * PLAIN,), 0xEE, dtype=torch.uint8, device=_dev(engine)),
            torch.full((n * FW,), 0xEE, dtype=torch.uint8, device=_dev(engine)),
            torch.full((n,), -7, dtype=torch.int32, device=_dev(engine)))


def _run(engine, t, pk, st, d_arena, epoch=EP, fw=True, status=True):
    import torch

    n = len(pk)
    d_plain, d_fw, d_in = _outputs(engine, n)
    O.inner_device(engine, t, _up(engine, pk), _up(engine, st).view(torch.int32), _up(engine, epoch).view(torch.int64), d_arena,
                   d_plain, d_fw if fw else None, d_in if status else None)
    torch.cuda.synchronize()
    return d_plain.cpu().numpy().tobytes(), d_fw.cpu().numpy().tobytes(), d_in.cpu().numpy().tolist()


def test_device_equals_host_equals_model(engine):
    case = RC.build()
    other = np.full(len(case.arena), 0x5A, np.uint8)  # the same packets, other bytes between them and in the tags
    for (off, ln) in case.packets:
        other[off:off + max(ln - 16, 0)] = case.arena[off:off + max(ln - 16, 0)]
    with PeerTable(engine, RC.CAPACITY) as t:
        RC.load(t, case)
        for n in SIZES:
            pk, st = RC.packet_arrays(case, n)
            want_plain, want_fw, want_st = RC.expected(case.model, case, n)
            h_plain, h_fw, h_st = O.inner_host(t, pk, st, EP, case.arena)
            assert (h_plain.tobytes(), h_fw.tobytes(), h_st.tolist()) == (want_plain, want_fw, want_st)
            for skew in range(4):
                d_arena = _up(engine, case.arena, skew)
                assert d_arena.data_ptr() % 4 == skew
                assert _run(engine, t, pk, st, d_arena) == (want_plain, want_fw, want_st), (n, skew)
                assert np.array_equal(d_arena.cpu().numpy(), case.arena)  # the input is only read
                # the other gap bytes, and without fw / without the status: the same records, nothing else written
                plain, fwb, ist = _run(engine, t, pk, st, _up(engine, other, skew), fw=skew % 2 == 1, status=skew < 2)
                assert plain == want_plain, (n, skew)
                assert fwb == (want_fw if skew % 2 == 1 else b"\xEE" * (n * FW))
                assert ist == (want_st if skew < 2 else [-7] * n)


def test_argument_checks(engine):
    import torch

    case = RC.build()
    lib = L.lib()
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    pk, st = RC.packet_arrays(case, 4)
    d_pk, d_st, d_ep, d_arena = _up(engine, pk), _up(engine, st), _up(engine, EP), _up(engine, case.arena)
    d_plain, d_fw, d_in = _outputs(engine, 4)
    args = lambda t, plain=d_plain, fw=d_fw: (engine.handle, t.handle, p(d_pk), p(d_st), p(d_ep), len(EP), 4, p(d_arena),  # noqa: E731
                                              plain if isinstance(plain, C.c_void_p) else p(plain),
                                              fw if isinstance(fw, C.c_void_p) else p(fw), p(d_in), None)
    with PeerTable(engine, 8) as t, PeerTable(None, 8) as host_only:
        assert lib.neb_rx_inner_batch(*args(host_only)) == L.ERR_INVALID  # nothing launched
        assert lib.neb_rx_inner_batch(*args(t, plain=C.c_void_p(d_plain.data_ptr() + 8))) == L.ERR_INVALID
        assert lib.neb_rx_inner_batch(*args(t, fw=C.c_void_p(d_fw.data_ptr() + 4))) == L.ERR_INVALID
        assert lib.neb_rx_inner_batch(engine.handle, t.handle, None, None, None, 0, 0, None, None, None, None, None) == L.OK
        assert lib.neb_rx_inner_batch(engine.handle, t.handle, None, p(d_st), p(d_ep), len(EP), 4, p(d_arena), p(d_plain), None,
                                      None, None) == L.ERR_INVALID
        torch.cuda.synchronize()
        assert (d_plain.cpu().numpy() == 0xEE).all() and (d_fw.cpu().numpy() == 0xEE).all() and (d_in.cpu().numpy() == -7).all()
        assert lib.neb_rx_inner_batch(*args(t)) == L.OK  # an empty table: every parsed packet is BAD_REMOTE
        torch.cuda.synchronize()
        assert set(d_in.cpu().numpy().tolist()) <= {M.BAD_REMOTE, M.INVALID, M.NOT_MESSAGE}


# ---- table states -----------------------------------------------------------------------------------

# Per tunnel: its VPN address and the same nest of prefixes, every length with another verdict than
# the one around it, so that each probe of the longest-prefix scan decides something.
NEST = [("0.0.0.0/0", L.NET_UNSAFE), ("128.0.0.0/1", L.NET_VPN_PEER), ("200.0.0.0/8", L.NET_UNSAFE), ("200.1.2.0/24", L.NET_VPN_PEER),
        ("200.1.2.4/31", L.NET_UNSAFE), ("200.1.2.5/32", L.NET_VPN_PEER), ("2001:db8:1::/48", L.NET_UNSAFE),
        ("2001:db8:1:2::/64", L.NET_VPN_PEER), ("2001:db8:1:2::4/127", L.NET_UNSAFE), ("2001:db8:1:2::5/128", L.NET_VPN_PEER)]
PROBES = [("9.9.9.9", M.OK), ("129.0.0.1", M.PEER_REJECTED), ("200.9.9.9", M.OK), ("200.1.2.9", M.PEER_REJECTED),
          ("200.1.2.4", M.OK), ("200.1.2.5", M.PEER_REJECTED), ("2001:db8:1:9::1", M.OK), ("2001:db8:1:2::9", M.PEER_REJECTED),
          ("2001:db8:1:2::4", M.OK), ("2001:db8:1:2::5", M.PEER_REJECTED), ("2001:db8:2::1", M.BAD_REMOTE)]


def _vpn(tunnel):
    return f"10.1.{16 + tunnel // 256}.{tunnel % 256}"


def _many(ntunnels):
    """PEER_NET_DTYPE for ntunnels tunnels x (VPN address + NEST), built without a Python loop per entry."""
    one = peer_nets([(0, p, ty) for p, ty in [("10.1.16.0/32", L.NET_VPN)] + NEST])
    nets = np.tile(one, ntunnels)
    tun = np.repeat(np.arange(ntunnels, dtype=np.uint32), len(one))
    nets["tunnel"] = tun
    own = np.arange(ntunnels) * len(one)
    nets["addr"][own, 2] = 16 + np.arange(ntunnels) // 256
    nets["addr"][own, 3] = np.arange(ntunnels) % 256
    return nets


def _probe_batch(tunnels, bare=None):
    """Per tunnel: its own address, another tunnel's address (the spoof), and PROBES -> items, arena,
    packets. 0.0.0.0/0 is in the nest, so the neighbour's address lies inside it, except for tunnel
    `bare`, which has no /0: there the address that is tunnel bare ^ 1's own /32 is refused."""
    items = []
    for t in tunnels:
        outside = M.BAD_REMOTE if t == bare else M.OK
        srcs = [(_vpn(t), M.OK), (_vpn(t ^ 1), outside), ("9.9.9.9", outside)] + PROBES[1:]
        for k, (src, want) in enumerate(srcs):
            p = RC.v6(RC.ME6, src=src) if ":" in src else RC.v4(RC.ME4, src=src, sport=k, dport=t % 65536)
            items.append((RC.wire(p, 1 + len(items)), t, want))
    arena, packets = bytearray(), []
    for w, _, _ in items:
        packets.append((len(arena), len(w)))
        arena += w + b"\xA5" * (1 + len(packets) % 3)
    return items, np.frombuffer(bytes(arena), np.uint8).copy(), packets


def _arrays(items, packets):
    pk = np.array([(off, ln, t) for (off, ln), (_, t, _) in zip(packets, items)], L.RX_PACKET_DTYPE)
    return pk, np.zeros(len(pk), np.int32)


@pytest.mark.parametrize("ntunnels", [1, 4096])
def test_table_of_many_tunnels(engine, ntunnels):
    nets = _many(ntunnels)
    sample = sorted({0, ntunnels - 1, ntunnels // 2} | set(random.Random(3).sample(range(ntunnels), min(ntunnels, 29))))
    model = M.Model()
    model.set_routable(routable(RC.MY_NETWORKS, RC.MY_UNSAFE))
    for t in sample:
        model.update((), [(t, _vpn(t) + "/32", L.NET_VPN)] + [(t, p, ty) for p, ty in NEST])
    bare = ntunnels // 2
    model.update([(bare, "0.0.0.0/0")], ())
    items, arena, packets = _probe_batch(sample, bare)
    assert sum(it[2] == M.BAD_REMOTE and it[1] == bare for it in items) == 3
    pk, st = _arrays(items, packets)
    epoch = np.arange(ntunnels, dtype=np.uint64) + (1 << 40)
    want = [model.inner(w, t, 0, epoch.tolist(), off=off) for (w, t, _), (off, _) in zip(items, packets)]
    assert [w[2] for w in want] == [it[2] for it in items]  # the nest decides as PROBES says
    with PeerTable(engine, 1 << 16) as t:
        t.set_routable(routable(RC.MY_NETWORKS, RC.MY_UNSAFE))
        t.update(put=nets)
        t.update(delete=[(bare, "0.0.0.0/0")])
        assert t.count() == len(nets) - 1
        got = _run(engine, t, pk, st, _up(engine, arena), epoch=epoch)
        h = O.inner_host(t, pk, st, epoch, arena)
        assert got == (h[0].tobytes(), h[1].tobytes(), h[2].tolist())
        assert got == (b"".join(w[0] for w in want), b"".join(w[1] for w in want), [w[2] for w in want])


def test_update_on_the_same_stream_and_compaction(engine):
    """Two calls with an update between them on one stream, no synchronisation in between: the first
    sees the table before it, the second after it. Then enough replacements to make the table
    compact itself into its spare image, and the same batch again."""
    import torch

    model = M.Model()
    model.set_routable(routable(RC.MY_NETWORKS, RC.MY_UNSAFE))
    base = [(t, _vpn(t) + "/32", L.NET_VPN) for t in range(4)] + [(t, p, ty) for t in range(4) for p, ty in NEST]
    model.update((), base)
    items, arena, packets = _probe_batch(range(4))
    pk, st = _arrays(items, packets)
    n = len(pk)
    epoch = np.arange(4, dtype=np.uint64) + 5
    d_pk, d_st, d_ep, d_arena = _up(engine, pk), _up(engine, st).view(torch.int32), _up(engine, epoch).view(torch.int64), _up(engine, arena)
    expect = lambda: [model.inner(w, t, 0, epoch.tolist(), off=off)[2] for (w, t, _), (off, _) in zip(items, packets)]  # noqa: E731
    with PeerTable(engine, 64) as t:
        t.set_routable(routable(RC.MY_NETWORKS, RC.MY_UNSAFE))
        t.update(put=base)
        before = expect()
        # the /24 of tunnel 1 goes (the /8 around it decides), tunnel 2's VPN address becomes a VPN_PEER, tunnel 3 gets a /16
        change = ([(1, "200.1.2.0/24"), (0, "2001:db8:1::/48")], [(2, _vpn(2) + "/32", L.NET_VPN_PEER), (3, "200.1.0.0/16", L.NET_VPN_PEER)])
        model.update(*change)
        after = expect()
        assert before != after
        outs = [_outputs(engine, n), _outputs(engine, n)]
        O.inner_device(engine, t, d_pk, d_st, d_ep, d_arena, *outs[0])
        t.update(*change)  # on the current stream, like the two calls
        O.inner_device(engine, t, d_pk, d_st, d_ep, d_arena, *outs[1])
        torch.cuda.synchronize()
        assert outs[0][2].cpu().numpy().tolist() == before
        assert outs[1][2].cpu().numpy().tolist() == after
        # every put takes a slot: 256 slots, so a few hundred replacements compact the table more than once
        last, rebuilds = 0, 0
        for k in range(300):
            t.update([(3, "200.1.0.0/16")] if k % 3 == 0 else (), [(3, "200.1.0.0/16", L.NET_VPN_PEER), (0, "77.0.0.0/8", 1 + k % 3)])
            probes = t.probe(0, "77.0.0.0/8")[2]
            rebuilds += probes < last
            last = probes
        assert rebuilds >= 2
        model.update((), [(0, "77.0.0.0/8", 1 + 299 % 3)])
        got = _run(engine, t, pk, st, d_arena, epoch=epoch)
        h = O.inner_host(t, pk, st, epoch, arena)
        assert got == (h[0].tobytes(), h[1].tobytes(), h[2].tolist()) and got[2] == expect() == after


# ---- between a real receive's open and its coalescer --------------------------------------------------

MARK = b"SPOOFED-PAYLOAD!"


def _traffic(rng, ntun, n):
    """[(tunnel, plaintext, typ, sub, forged, want)]: TCP flows from each tunnel's peer, with spoofed
    sources, wrong destinations, malformed inner packets, Test packets and forged tags among them."""
    out, seq = [], [1000] * ntun
    peer = lambda t: f"10.1.0.{20 + t}"  # noqa: E731
    for i in range(n):
        t = i * ntun // n if i % 5 else rng.randrange(ntun)
        body = bytes([i & 255]) * 120
        kind = "spoof" if i % 11 == 3 else "misdirected" if i % 13 == 5 else "malformed" if i % 17 == 7 else \
            "test" if i % 19 == 9 else "forged" if i % 23 == 11 else "good"
        src, dst, want = peer(t), RC.ME4, M.OK
        if kind == "spoof":
            src, body, want = peer((t + 1) % ntun), MARK * 8, M.BAD_REMOTE
        elif kind == "misdirected":
            dst, want = "10.1.0.8", M.BAD_LOCAL
        p = RC.tcp4(src, dst, seq[t], body, sport=40000 + t)
        if kind == "good":  # the committed segments of a tunnel are one gapless flow
            seq[t] += len(body)
        if kind == "malformed":
            p, want = p[:22], M.INVALID
        if kind in ("test", "forged"):
            want = M.NOT_MESSAGE
        out.append((t, p, (4, 0) if kind == "test" else (1, 0), kind == "forged", want, kind))
    return out


def _receive_check(engine, alg, table, pkt, arena, epoch, d_pk, d_ist, d_arena, want, kinds):
    """inner + coalesce on the device over opened records (d_pk, d_ist) == the host forms over the
    arena the device opened; statuses as the traffic says; no spoofed byte in any write."""
    import torch

    n = len(pkt)
    dev = _dev(engine)
    cap = int(((pkt["len"].astype(np.int64) + 15) & ~15).sum())
    d_plain, d_fw, d_in = _outputs(engine, n)
    d_out = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
    d_writes = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_nw, d_pw, d_ps = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (1, n, n))
    O.inner_device(engine, table, d_pk, d_ist, _up(engine, epoch).view(torch.int64), d_arena, d_plain, d_fw, d_in)
    O.coalesce_batch_device(engine, d_plain, d_arena, d_out[:cap], d_writes, d_nw, d_pw, d_ps)
    torch.cuda.synchronize(dev)
    inner = d_in.cpu().numpy()
    assert inner.tolist() == want
    opened = d_arena.cpu().numpy()
    pk, ist = d_pk.cpu().numpy().view(L.RX_PACKET_DTYPE), d_ist.cpu().numpy()
    h_plain, h_fw, h_in = O.inner_host(table, pk, ist, epoch, opened)
    assert (d_plain.cpu().numpy().tobytes(), d_fw.cpu().numpy().tobytes()) == (h_plain.tobytes(), h_fw.tobytes())
    assert h_in.tolist() == want
    writes, out, pw, ps = O.coalesce_batch_host(h_plain, opened, out_cap=cap, max_writes=n)
    nw = int(d_nw.item())
    assert nw == len(writes) and d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:nw].tobytes() == writes.tobytes()
    used = int(writes[-1]["out_off"]) + int(writes[-1]["len"])
    got_out = d_out.cpu().numpy()
    assert got_out[:used].tobytes() == out[:used].tobytes()
    assert d_pw.cpu().numpy().view(np.uint32).tolist() == pw.tolist() and d_ps.cpu().numpy().tolist() == ps.tolist()
    assert MARK not in got_out.tobytes() and MARK in opened.tobytes()  # opened, and then not committed
    for i, k in enumerate(kinds):
        assert (pw[i] != L.WRITE_NONE) == (k == "good"), (i, k)
    assert max(int(w["nseg"]) for w in writes) >= 5  # and the good segments still coalesce around the gaps


@pytest.mark.parametrize("alg", [L.ALG_AESGCM, L.ALG_CHACHAPOLY])
@pytest.mark.parametrize("relayed", [False, True])
def test_between_a_real_open_and_the_coalescer(engine, oracle_mod, alg, relayed):
    import torch

    import relay_forward_ref as R
    import rx_via_ref as V
    from nebula_amd.connection_state import Bits, DeviceWindows
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly
    from nebula_amd.relay import rx_open_via_batch_device

    rng = random.Random(60 + alg)
    ntun = 3
    keys = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(ntun + 1)]  # the last one: the relay
    cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
    ciphers = [cf.Cipher(engine, k) for k in keys]
    dw = None
    try:
        traffic = _traffic(rng, ntun, 300)
        ctr, rctr = [10] * ntun, 50
        arena, pk = bytearray(b"\0" * 3), []
        for t, p, (typ, sub), forged, _, _ in traffic:
            ctr[t] += 1
            wire = bytearray(R.seal_message(oracle_mod, alg, keys[t], 0x100 + t, ctr[t], p, typ, sub))
            if forged:
                wire[-1] ^= 1
            if relayed:
                rctr += 1
                wire = V.seal_relay(oracle_mod, alg, keys[ntun], 0x1FF, rctr, bytes(wire))
            pk.append((len(arena), len(wire), ciphers[ntun if relayed else t].key_id))
            arena += wire + b"\0" * (len(pk) % 4)
        n = len(pk)
        pkt = np.array(pk, L.RX_PACKET_DTYPE)
        epoch = np.zeros(max(c.key_id for c in ciphers) + 1, np.uint64)
        for t in range(ntun):
            epoch[ciphers[t].key_id] = 40 + t
        dw = DeviceWindows(engine, engine.max_keys, 1024)
        for c in ciphers:
            w = Bits(1024)
            dw.load(c.key_id, w)
            w.destroy()
        want = [w for _, _, _, _, w, _ in traffic]
        kinds = [k for *_, k in traffic]
        with PeerTable(engine, 16) as table:
            table.set_routable(routable(RC.MY_NETWORKS, RC.MY_UNSAFE))
            table.update(put=[(ciphers[t].key_id, f"10.1.0.{20 + t}/32", L.NET_VPN) for t in range(ntun)])
            d_pk, d_arena = _up(engine, pkt), _up(engine, np.frombuffer(bytes(arena), np.uint8))
            d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev(engine))
            if not relayed:
                from nebula_amd.connection_state import rx_open_wire_batch_device

                rx_open_wire_batch_device(engine, alg, dw, d_pk, d_arena, d_st, L.KEYS_MIXED, None)
                d_opened, d_ist = d_pk, d_st
            else:
                via = np.array([(ciphers[t].key_id, L.VIA_TERMINAL) for t, *_ in traffic], L.RX_VIA_DTYPE)
                d_opened = torch.zeros(n * 16, dtype=torch.uint8, device=_dev(engine))
                d_ist = torch.full((n,), -1, dtype=torch.int32, device=_dev(engine))
                rx_open_via_batch_device(engine, alg, dw, d_pk, _up(engine, via), d_arena, d_st, d_opened, d_ist)
                torch.cuda.synchronize()
                assert (d_st.cpu().numpy() == 0).all()
            _receive_check(engine, alg, table, pkt, arena, epoch, d_opened, d_ist, d_arena, want, kinds)
    finally:
        if dw is not None:
            dw.destroy()
        for c in ciphers:
            c.destroy()


def test_receive_takes_a_peer_table(engine, oracle_mod):
    """outside.receive with `peers` runs the new call in neb_rx_plain_from_wire's place; without it the
    composition is the old one and commits the spoofed packet."""
    import torch

    import relay_forward_ref as R
    from nebula_amd.connection_state import Bits, DeviceWindows
    from nebula_amd.noiseutil import CipherAESGCM

    alg = L.ALG_AESGCM
    key = bytes(range(32))
    c = CipherAESGCM.Cipher(engine, key)
    dw = None
    try:
        inner = [RC.tcp4("10.1.0.20", RC.ME4, 1, b"a" * 50), RC.tcp4("10.1.0.21", RC.ME4, 1, MARK * 4), RC.tcp4("10.1.0.20", RC.ME4, 51, b"b" * 50)]
        arena, pk = bytearray(), []
        for i, p in enumerate(inner):
            w = R.seal_message(oracle_mod, alg, key, 0x100, 11 + i, p)
            pk.append((len(arena), len(w), c.key_id))
            arena += w
        pkt = np.array(pk, L.RX_PACKET_DTYPE)
        epoch = np.zeros(c.key_id + 1, np.uint64)
        dev = _dev(engine)
        results = []
        with PeerTable(engine, 4) as table:
            table.set_routable(routable(RC.MY_NETWORKS))
            table.update(put=[(c.key_id, "10.1.0.20/32", L.NET_VPN)])
            for peers in (None, table):
                dw = DeviceWindows(engine, engine.max_keys, 64)
                w = Bits(64)
                dw.load(c.key_id, w)
                w.destroy()
                d_pk, d_arena = _up(engine, pkt), _up(engine, np.frombuffer(bytes(arena), np.uint8))
                d_st = torch.full((3,), -1, dtype=torch.int32, device=dev)
                d_plain, d_fw, d_in = _outputs(engine, 3)
                d_out = torch.zeros(1024, dtype=torch.uint8, device=dev)
                d_writes = torch.zeros(3 * 32, dtype=torch.uint8, device=dev)
                d_nw, d_pw, d_ps = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (1, 3, 3))
                O.receive(engine, alg, dw, d_pk, d_arena, d_st, _up(engine, epoch).view(torch.int64), d_plain, d_out, d_writes,
                          d_nw, d_pw, d_ps, peers=peers, d_fw=d_fw, d_inner_status=d_in)
                torch.cuda.synchronize()
                dw.destroy()
                dw = None
                assert d_st.cpu().numpy().tolist() == [0, 0, 0]
                results.append((d_pw.cpu().numpy().view(np.uint32).tolist(), d_out.cpu().numpy().tobytes(), d_in.cpu().numpy().tolist(),
                                d_fw.cpu().numpy().view(L.FW_PACKET_DTYPE)))
        (pw0, out0, in0, _), (pw1, out1, in1, fw1) = results
        assert L.WRITE_NONE not in pw0 and MARK in out0 and in0 == [-7] * 3  # the old path commits everything
        assert pw1[1] == L.WRITE_NONE and pw1[0] == pw1[2] != L.WRITE_NONE and MARK not in out1
        assert in1 == [M.OK, M.BAD_REMOTE, M.OK]
        assert bytes(fw1[1]["remote_addr"][:4]) == ipaddress.ip_address("10.1.0.21").packed  # what rejectOutside needs
    finally:
        if dw is not None:
            dw.destroy()
        c.destroy()
