"""GPU: the transmit batch through relays (neb_tx_seal_via_batch[_host] — sendInsideMessage with its
relay branch, inside.go:178-223, and prepareSendVia, :442-501) against the sequential model in
tests/tx_via_ref.py, against neb_tx_seal_batch, and through the engine's own relay forwarding and
receive. Every check is bit-exact."""
import random

import numpy as np
import pytest

import tx_via_ref as M
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

from test_gpu_relay_forward import _Node, _keys  # noqa: E402
from test_gpu_tx import _pk, _to_arrays, _tunnels, build_udpv6_super  # noqa: E402
from test_segment_oracle import build_tcpv4_super, build_tcpv6_super, build_udpv4_single, build_udpv4_super  # noqa: E402

ALGS = [L.ALG_AESGCM, L.ALG_CHACHAPOLY]
NONE = M.RELAY_NONE


def _via_array(via):
    return None if via is None else np.array(via, dtype=L.RELAY_ROUTE_DTYPE)


class _Keys:
    """The tunnels' keys installed on the engine for one test."""

    def __init__(self, engine, alg, tun_spec):
        from nebula_amd.inside import TX_TUNNEL_DTYPE
        from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

        cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
        self.ciphers = [cf.Cipher(engine, t["key"]) if t["key"] is not None else None for t in tun_spec]
        self.tun = np.zeros(len(tun_spec), TX_TUNNEL_DTYPE)
        for i, (t, c) in enumerate(zip(tun_spec, self.ciphers)):
            self.tun[i] = (t["counter"], c.key_id if c is not None else L.KEYS_MIXED, t["remote_index"])

    def close(self):
        for c in self.ciphers:
            if c is not None:
                c.destroy()


def _run(engine, alg, tun, via, pk, arena, out_cap, max_wires, device, hint=L.KEYS_MIXED, direct=False):
    """One batch through neb_tx_seal_via_batch[_host] (direct: through neb_tx_seal_batch[_host])."""
    from nebula_amd.inside import DeviceTxBatch, tx_seal_batch_host, tx_seal_via_batch_host

    if device:
        import torch

        db = DeviceTxBatch(engine, alg, tun, pk, arena, out_cap, max_wires, hint, via=None if direct else via)
        if not direct and via is None:  # the via call itself, with a NULL array
            rc = L.lib().neb_tx_seal_via_batch(
                engine.handle, alg, db.tunnels.data_ptr(), db.ntun, None, db.packets.data_ptr(), db.npk,
                db.inp.data_ptr(), db.out.data_ptr(), db.out.numel(), db.wires.data_ptr(), db.wire_status.data_ptr(),
                max_wires, db.nwires.data_ptr(), db.pk_status.data_ptr(), hint,
                torch.cuda.current_stream().cuda_stream)
            L.check(rc, "neb_tx_seal_via_batch")
        else:
            db.seal()
        torch.cuda.synchronize()
        return db.result()
    if direct:
        return tx_seal_batch_host(engine, alg, tun, pk, arena, out_cap, max_wires, hint)
    return tx_seal_via_batch_host(engine, alg, tun, via, pk, arena, out_cap, max_wires, hint)


def _check(engine, oracle_mod, alg, packets, tun_spec, via, out_cap=1 << 20, max_wires=4096, device=False,
           key_hint=None, skew=None):
    """The batch against the model: statuses, wire records, the bytes of every OK wire, counters."""
    K = _Keys(engine, alg, tun_spec)
    try:
        pk, arena = _to_arrays(packets, skew)
        exp_w, exp_pst, exp_ctr = M.tx_via_batch(alg, tun_spec, via, packets, out_cap, max_wires,
                                                 M.oracle_seal(oracle_mod), oracle_mod.header_encode)
        hint = L.KEYS_MIXED if key_hint is None else K.ciphers[key_hint].key_id
        r = _run(engine, alg, K.tun, _via_array(via), pk, arena, out_cap, max_wires, device, hint)
        assert r.packet_status.tolist() == exp_pst
        assert len(r.wires) == len(exp_w)
        for i, (off, c, ln, p, j, st, flag, data) in enumerate(exp_w):
            w = r.wires[i]
            assert (int(w["out_off"]), int(w["counter"]), int(w["len"]), int(w["packet"]), int(w["segment"]),
                    int(w["reserved"])) == (off, c, ln, p, j, flag), i
            assert int(r.wire_status[i]) == st, i
            if data is not None:
                assert r.wire_bytes(i) == data, (i, p, j)
        assert r.tunnels["message_counter"].tolist() == exp_ctr
        return r, exp_w
    finally:
        K.close()


def _shapes(S, rng):
    """One read of every shape, as (data, flags, gso_type, gso_size, csum_start, csum_offset)."""
    tcp, _, cs = build_tcpv4_super(2500)       # 3 segments, the last one short
    tcp6, _, cs6 = build_tcpv6_super(3001)
    udp, _, csu = build_udpv4_super(2500)
    udp6, _, csu6 = build_udpv6_super(777)
    plain = [(bytes(rng.getrandbits(8) for _ in range(n)), 0, 0, 0, 0, 0) for n in (1, 20, 576, 1300, 9000)]
    return plain + [
        (build_udpv4_single(S, b"finish me please" * 5), S.F_NEEDS_CSUM, 0, 0, 20, 6),
        (tcp, 1, S.GSO_TCPV4, 1000, cs, 16),
        (tcp6, 1, S.GSO_TCPV6, 1000, cs6, 16),
        (udp, 1, S.GSO_UDP_L4, 1200, csu, 6),
        (udp6, 1, S.GSO_UDP_L4, 300, csu6, 6),
        (tcp, 1, S.GSO_TCPV4, 0, cs, 16),      # gso_size 0: CheckValid refuses it
    ]


# T0 direct and the relay of T1; T2 via T3; T3 direct; T4 via keyless T5; T6 via an index out of
# range; T7 via T1, which itself has a via; T8 via itself; T9 keyless, with a valid via
PARITY_VIA = [(NONE, 0), (0, 0x7100), (3, 0x7200), (NONE, 0), (5, 0x7400), (NONE, 0), (99, 0x7600), (1, 0x7700),
              (8, 0x7800), (0, 0x7900)]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("alg", ALGS)
def test_tx_via_matches_sequential_model(engine, oracle_mod, alg, device):
    import segment_oracle as S

    rng = random.Random(20 * alg + device)
    shapes = _shapes(S, rng)
    P = []
    for k in range(44):  # every shape on every tunnel kind over the four rounds
        d, fl, gt, gs, cs, co = shapes[k % len(shapes)]
        P.append(_pk(d, [0, 1, 2, 3, 1, 0, 2, 1][(k + k // 11) % 8] if k % 5 else 4 + (k // 5) % 6, fl, gt, gs, cs, co))
    rng.shuffle(P)
    tun = _tunnels(rng, n=10, keyless=(5, 9))
    r, exp_w = _check(engine, oracle_mod, alg, P, tun, PARITY_VIA, out_cap=1 << 20, max_wires=512, device=device)
    assert {L.STATUS_OK, L.STATUS_BAD_KEY, L.STATUS_INVALID} <= set(r.packet_status.tolist())
    assert {0, L.TX_WIRE_VIA} == set(r.wires["reserved"].tolist())
    for t in (4, 6, 7, 8, 9):
        assert all(st != L.STATUS_OK for st, p in zip(r.packet_status, P) if p["tunnel"] == t)


@pytest.mark.parametrize("device", [False, True])
def test_tx_via_without_relays_is_tx_seal_batch(engine, oracle_mod, device):
    """via all NEB_RELAY_NONE, and via NULL: the arena, the wires, the statuses and the counters of
    neb_tx_seal_batch on the same input."""
    import segment_oracle as S

    alg = L.ALG_AESGCM
    rng = random.Random(31 + device)
    shapes = _shapes(S, rng)
    P = [_pk(shapes[k % len(shapes)][0], k % 4, *shapes[k % len(shapes)][1:]) for k in range(26)]
    tun = _tunnels(rng, n=4, keyless=(3,))
    K = _Keys(engine, alg, tun)
    try:
        pk, arena = _to_arrays(P)
        want = _run(engine, alg, K.tun, None, pk, arena, 1 << 18, 256, device, direct=True)
        assert len(want.wires) > 30
        for via in (_via_array([(NONE, 5)] * 4), None):
            got = _run(engine, alg, K.tun, via, pk, arena, 1 << 18, 256, device)
            assert np.array_equal(got.out, want.out)
            assert got.wires.tobytes() == want.wires.tobytes()
            assert np.array_equal(got.wire_status, want.wire_status)
            assert np.array_equal(got.packet_status, want.packet_status)
            assert got.tunnels.tobytes() == want.tunnels.tobytes()
    finally:
        K.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("alg", ALGS)
def test_tx_via_counter_order(engine, oracle_mod, alg, device):
    """Reads alternate "direct to R" and "to T via R": R's counters, read from the first header of
    every wire, and T's, from the inner headers, are contiguous in batch order."""
    import segment_oracle as S

    rng = random.Random(41)
    tun = _tunnels(rng, n=2, keyless=())  # R = 0, T = 1
    tcp, _, cs = build_tcpv4_super(2500)
    P = []
    for k in range(9):
        if k == 4:
            P.append(_pk(tcp, 1, 1, S.GSO_TCPV4, 1000, cs, 16))  # 3 segments via R
        elif k == 7:
            P.append(_pk(tcp, 0, 1, S.GSO_TCPV4, 1000, cs, 16))  # 3 segments direct to R
        else:
            P.append(_pk(bytes(rng.getrandbits(8) for _ in range(30 + k)), k & 1))
    r, _ = _check(engine, oracle_mod, alg, P, tun, [(NONE, 0), (0, 0x99)], device=device)
    assert len(r.wires) == 13
    first = [int.from_bytes(r.wire_bytes(i)[8:16], "big") for i in range(13)]
    assert first == list(range(tun[0]["counter"] + 1, tun[0]["counter"] + 14))
    inner = [int.from_bytes(r.wire_bytes(i)[24:32], "big") for i in range(13) if r.wires[i]["reserved"]]
    assert inner == list(range(tun[1]["counter"] + 1, tun[1]["counter"] + 7))
    assert inner == [int(w["counter"]) for w in r.wires if w["reserved"]]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("who", ["target", "relay"])
def test_tx_via_exhaustion(engine, oracle_mod, who, device):
    """Six one-segment via reads. The target at REJECT_AFTER - 3: two wires, four EXHAUSTED that take
    no outer counter. The relay at REJECT_AFTER - 3: all six inner counters used, two wires, the
    relay's six counters used."""
    import segment_oracle as S

    rng = random.Random(51)
    tun = _tunnels(rng, n=2, keyless=())
    t = 1 if who == "target" else 0
    tun[t]["counter"] = S.REJECT_AFTER - 3
    start = [x["counter"] for x in tun]
    P = [_pk(bytes(rng.getrandbits(8) for _ in range(40 + k)), 1) for k in range(6)]
    r, _ = _check(engine, oracle_mod, L.ALG_AESGCM, P, tun, [(NONE, 0), (0, 0x99)], device=device)
    assert r.wire_status.tolist() == [0, 0, 2, 2, 2, 2]
    adv = [int(c) - s for c, s in zip(r.tunnels["message_counter"], start)]
    assert adv == ([2, 6] if who == "target" else [6, 6])


@pytest.mark.parametrize("device", [False, True])
def test_tx_via_capacity_prefix(engine, oracle_mod, device):
    """An output that holds the batch at direct slot sizes but not at via sizes keeps the longest
    fitting prefix; the other reads are NO_SPACE and use no counter on either tunnel."""
    import segment_oracle as S

    rng = random.Random(61)
    shapes = _shapes(S, rng)[:10]
    P = [_pk(shapes[k % 10][0], 1 + (k & 1), *shapes[k % 10][1:]) for k in range(20)]
    tun = _tunnels(rng, n=3, keyless=())
    via = [(NONE, 0), (0, 0x31), (NONE, 0)]
    seal = M.oracle_seal(oracle_mod)
    direct_w, _, _ = S.tx_batch(L.ALG_AESGCM, tun, P, 1 << 30, 4096, seal, oracle_mod.header_encode)
    out_cap = sum(S.slot_bytes(w[2] - 32) for w in direct_w)
    r, exp_w = _check(engine, oracle_mod, L.ALG_AESGCM, P, tun, via, out_cap=out_cap, device=device)
    assert 0 < len(exp_w) < len(direct_w)
    assert L.STATUS_NO_SPACE in r.packet_status.tolist()
    used = {1: sum(1 for w in exp_w if w[6]), 2: sum(1 for w in exp_w if not w[6])}
    assert [int(c) for c in r.tunnels["message_counter"]] == [tun[0]["counter"] + used[1], tun[1]["counter"] + used[1],
                                                              tun[2]["counter"] + used[2]]


@pytest.mark.parametrize("n", [1025, 2049, 8193])
def test_tx_via_plan_sizes(engine, oracle_mod, n):
    """The smallest batches that reach 2 and 8 reads per thread of the one-workgroup plan and the
    grid-wide plan: one-segment reads over 64 tunnels, half of them via 4 relays with uneven shares."""
    rng = random.Random(n)
    tun = _tunnels(rng, n=64, keyless=(17,))
    via = [(NONE, 0)] * 32 + [(min(int(rng.expovariate(0.9)), 3), 0x4000 + t) for t in range(32, 64)]
    P = [_pk(bytes(rng.getrandbits(8) for _ in range(rng.randrange(20, 61))), rng.randrange(64)) for _ in range(n)]
    for k in range(0, n, 97):
        P[k] = _pk(b"", P[k]["tunnel"])  # a short tun read
    r, _ = _check(engine, oracle_mod, L.ALG_AESGCM, P, tun, via, out_cap=n * 128, max_wires=16384, device=True)
    nvia = int((r.wires["reserved"] == L.TX_WIRE_VIA).sum())
    assert 0.35 * n < nvia < 0.65 * n


@pytest.mark.parametrize("alg", ALGS)
def test_tx_via_chain(engine, oracle_mod, alg):
    """What the via batch wrote travels: the relay node's neb_relay_forward_batch (inbound key = the
    relay tunnel's) forwards every wire, the target's receive verifies the forwarded packets, and the
    inner packets open under the target tunnel's key to the segments of the reads (no model)."""
    import segment_oracle as S

    rng = random.Random(71 + alg)
    k_relay, k_target, k_hop = _keys(rng, 3)
    tun = [dict(counter=10, remote_index=0x111, key=k_relay), dict(counter=20, remote_index=0x222, key=k_target)]
    shapes = _shapes(S, rng)[:10]
    P = [_pk(shapes[k % 10][0], 1, *shapes[k % 10][1:]) for k in range(20)]
    segs = [s for p in P for s in S.segment_superpacket(p["data"], p["flags"], p["gso_type"], p["hdr_len"],
                                                        p["gso_size"], p["csum_start"], p["csum_offset"])]
    K = _Keys(engine, alg, tun)
    relay = _Node(engine, alg, [k_relay], [k_hop])
    target = _Node(engine, alg, [k_hop, k_target], [])
    try:
        pk, arena = _to_arrays(P)
        r = _run(engine, alg, K.tun, _via_array([(NONE, 0), (0, 0x333)]), pk, arena, 1 << 18, 256, True)
        assert len(r.wires) == len(segs) and (r.wire_status == 0).all() and (r.wires["reserved"] == 1).all()
        wires = [(int(w["out_off"]), int(w["len"]), 0) for w in r.wires]
        routes = [(0, 0x444)] * len(wires)
        st, fwd, out, _, rt = relay.run(True, wires, routes, relay.tunnels([5]), r.out, 1024)
        assert (st == 0).all() and (fwd == 0).all() and int(rt["message_counter"][0]) == 5 + len(wires)
        st2, _, out2, _, _ = target.run(True, wires, routes, target.tunnels([]), out, 1024, forward=False)
        assert (st2 == 0).all()  # VerifyRelay under the hop key
        inner = [(off + 16, ln - 32, 1) for off, ln, _ in wires]
        st3, _, out3, _, _ = target.run(True, inner, routes, target.tunnels([]), out2, 1024, forward=False)
        assert (st3 == 0).all()
        for (off, ln, _), seg in zip(inner, segs):
            assert bytes(out3[off + 16:off + ln - 16]) == seg
    finally:
        K.close()
        relay.close()
        target.close()


def test_tx_via_shares_counters_with_tx_batch_and_forwarding(engine, oracle_mod):
    """neb_tx_seal_batch, a via batch and a forward on one tunnel array and stream: each tunnel's
    counters are contiguous across the three and none repeats."""
    import torch

    from nebula_amd.connection_state import DeviceWindows
    from nebula_amd.inside import TX_PACKET_DTYPE, DeviceTxBatch
    from nebula_amd.relay import relay_forward_batch_device
    import relay_forward_ref as F

    alg = L.ALG_AESGCM
    rng = random.Random(81)
    in_keys, tun_keys = _keys(rng, 1), _keys(rng, 2)
    node = _Node(engine, alg, in_keys, tun_keys)
    try:
        start = [100, 7000]
        tun = node.tunnels(start)  # tunnel 0 = R, tunnel 1 = T (via R in the via batch)
        ntx = 10
        txp = np.zeros(ntx, TX_PACKET_DTYPE)
        for i in range(ntx):
            txp[i] = (i * 64, 40 + i, i % 2, 0, 0, 0, 0, 0, 0, 0)
        reads = np.frombuffer(bytes(rng.getrandbits(8) for _ in range(ntx * 64)), np.uint8)
        db = DeviceTxBatch(engine, alg, tun, txp, reads, 1 << 16, 64)
        dv = DeviceTxBatch(engine, alg, tun, txp, reads, 1 << 16, 64, via=_via_array([(NONE, 0), (0, 0x55)]))
        dv.tunnels = db.tunnels  # one tunnel array
        nfw = 9
        pkts = [(F.seal_relay(oracle_mod, alg, in_keys[0], 1, 3 + i, b"q" * i), 0) for i in range(nfw)]
        routes = [(0 if i % 3 else 1, 0x33) for i in range(nfw)]
        arena = np.zeros(nfw * 64, np.uint8)
        packets = []
        for i, (p, t) in enumerate(pkts):
            arena[i * 64:i * 64 + len(p)] = np.frombuffer(p, np.uint8)
            packets.append((i * 64, len(p), t))
        dev = torch.device("cuda", engine.device)
        dw = DeviceWindows(engine, engine.max_keys, 64)
        try:
            dw.load(node.cin[0].key_id, node.windows(64)[0])
            up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)  # noqa: E731
            d_pk, d_rt, d_arena = up(node.rx_packets(packets)), up(np.array(routes, dtype=L.RELAY_ROUTE_DTYPE)), up(arena)
            d_st = torch.full((nfw,), -1, dtype=torch.int32, device=dev)
            d_fwd = torch.full((nfw,), -1, dtype=torch.int32, device=dev)
            db.seal()
            dv.seal()
            relay_forward_batch_device(engine, alg, dw, d_pk, d_rt, db.tunnels, d_arena, d_st, d_fwd)
            torch.cuda.synchronize()
            r1, r2 = db.result(), dv.result()
            out = d_arena.cpu().numpy()
            assert (d_fwd.cpu().numpy() == 0).all()
        finally:
            dw.destroy()
        used = {0: [], 1: []}
        for w in r1.wires:
            used[int(txp[int(w["packet"])]["tunnel"])].append(int(w["counter"]))
        for i, w in enumerate(r2.wires):
            if w["reserved"]:
                used[1].append(int(w["counter"]))
                used[0].append(int.from_bytes(r2.wire_bytes(i)[8:16], "big"))
            else:
                used[0].append(int(w["counter"]))
        for i, (off, _, _) in enumerate(packets):
            used[routes[i][0]].append(int.from_bytes(bytes(out[off + 8:off + 16]), "big"))
        for t in (0, 1):
            assert used[t] == list(range(start[t] + 1, start[t] + 1 + len(used[t]))), (t, used[t])
            assert int(r2.tunnels[t]["message_counter"]) == start[t] + len(used[t])
        assert len(used[0]) + len(used[1]) == 2 * ntx + ntx // 2 + nfw
    finally:
        node.close()


@pytest.mark.parametrize("alg,grid", [(L.ALG_AESGCM, None), (L.ALG_AESGCM, 1), (L.ALG_CHACHAPOLY, None)])
def test_tx_via_one_relay_one_target_key(engine, oracle_mod, alg, grid, knobs):
    """key_hint = the target's key and one relay: both seals run as single-key launches (AES-GCM:
    the inner one sums the payloads into the L4 checksums). 273 wires: one packet past a multiple
    of 16, and with `grid` a 1-workgroup seal grid leaves them to its tail kernel."""
    import segment_oracle as S

    if grid is not None:
        knobs(L.KNOB_SINGLE_MAX_GRID, grid)
    rng = random.Random(91 + alg)
    tun = _tunnels(rng, n=2, keyless=())
    P = []
    for i in range(30):  # 9 segments each
        if i % 3 == 0:
            d, _, cs = build_tcpv4_super(8 * 1000 + rng.randrange(1, 1000))
            P.append(_pk(d, 1, 1, S.GSO_TCPV4, 1000, cs, 16))
        elif i % 3 == 1:
            d, _, cs = build_tcpv6_super(8 * 900 + rng.randrange(1, 900))
            P.append(_pk(d, 1, 1, S.GSO_TCPV6, 900, cs, 16))
        else:
            d, _, cs = build_udpv4_super(8 * 1200 + rng.randrange(1, 1200))
            P.append(_pk(d, 1, 1, S.GSO_UDP_L4, 1200, cs, 6))
    P.append(_pk(build_udpv4_single(S, b"finish me please" * 5), 1, S.F_NEEDS_CSUM, 0, 0, 20, 6))
    P += [_pk(bytes(rng.getrandbits(8) for _ in range(n)), 1) for n in (1, 777)]
    r, _ = _check(engine, oracle_mod, alg, P, tun, [(NONE, 0), (0, 0x66)], out_cap=1 << 20, max_wires=512,
                  device=True, key_hint=1, skew=[0, 4, 8, 3])
    assert len(r.wires) == 273 and (r.wires["reserved"] == 1).all()
