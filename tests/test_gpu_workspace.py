"""GPU: the engine's device workspaces (nebula_amd/csrc/workspace.hpp) across two streams. Each case
runs two batches of one entry point on two different streams of a fresh engine with no host
synchronisation between them; the second batch is the one that makes the workspace grow (past the
floor its first allocation has), so the workspace is freed, allocated and laid out again while the
first batch may still be queued. Both batches' complete outputs, in separate buffers and read only
after both streams are synchronized, equal the reference models bit for bit. Nothing here depends
on timing: tests/sanitize/workspace_test.cpp pins the ordering calls themselves; these cases catch
the use of a freed or re-laid-out workspace."""
import ctypes as C
import random

import numpy as np
import pytest

import coalesce_cases as K
import coalesce_ref as CM
import relay_forward_ref as RM
import tx_via_ref as TM
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

from test_gpu_relay_forward import _Node, _keys, _lay_out  # noqa: E402
from test_gpu_tx import _pk, _to_arrays, _tunnels  # noqa: E402
from test_gpu_tx_via import _Keys, _via_array  # noqa: E402
from test_segment_oracle import build_tcpv4_super  # noqa: E402


@pytest.fixture
def fresh():
    """An engine of the test's own: its workspaces start empty (the session's engine has grown its
    own in earlier tests)."""
    from nebula_amd import Engine

    e = Engine(0, max_keys=256)
    yield e
    for cs in list(e.live.values()):
        cs.destroy()
    e.close()


def _two_streams():
    import torch

    torch.cuda.synchronize()  # the uploads and fills of both batches, before either stream starts
    return torch.cuda.Stream(), torch.cuda.Stream()


def _tx_packets(rng, n, ntun):
    """n TUN reads over ntun tunnels: plain reads of 40-200 B and a TSO superpacket every 97th."""
    import segment_oracle as S

    tcp, _, cs = build_tcpv4_super(2500)
    P = []
    for i in range(n):
        if i % 97 == 5:
            P.append(_pk(tcp, i % ntun, 1, S.GSO_TCPV4, 1000, cs, 16))
        else:
            P.append(_pk(bytes(rng.getrandbits(8) for _ in range(rng.randrange(40, 200))), i % ntun))
    return P


@pytest.mark.parametrize("via", [False, True], ids=["neb_tx_seal_batch", "neb_tx_seal_via_batch"])
def test_tx_workspace_grows_under_a_queued_batch(fresh, oracle_mod, via):
    """64 reads over 2 tunnels on stream A, then 1500 over 80 on stream B: past the 1024-packet,
    64-tunnel and 1024-wire floors of the first allocation."""
    import torch

    from nebula_amd.inside import DeviceTxBatch

    alg = L.ALG_AESGCM
    rng = random.Random(41 + via)
    shapes = [(64, 2, 128, 1 << 16), (1500, 80, 2048, 1 << 20)]  # reads, tunnels, max_wires, out_cap
    held, runs = [], []
    try:
        for n, ntun, max_wires, out_cap in shapes:
            tun = _tunnels(rng, n=ntun, keyless=())
            # tunnel 0 (and 1-3 of the large batch) are reached directly and relay the others
            nrelay = 1 if ntun == 2 else 4
            routes = [(TM.RELAY_NONE, 0) if t < nrelay else (t % nrelay, 0x7000 + t) for t in range(ntun)] if via else None
            P = _tx_packets(rng, n, ntun)
            keys = _Keys(fresh, alg, tun)
            held.append(keys)
            pk, arena = _to_arrays(P)
            exp = TM.tx_via_batch(alg, tun, routes, P, out_cap, max_wires, TM.oracle_seal(oracle_mod),
                                  oracle_mod.header_encode)
            db = DeviceTxBatch(fresh, alg, keys.tun, pk, arena, out_cap, max_wires, L.KEYS_MIXED, via=_via_array(routes))
            runs.append((db, exp))
        streams = _two_streams()
        for (db, _), s in zip(runs, streams):
            with torch.cuda.stream(s):
                db.seal()
        for s in streams:
            s.synchronize()
        for db, (exp_w, exp_pst, exp_ctr) in runs:
            r = db.result()
            assert r.packet_status.tolist() == exp_pst
            assert len(r.wires) == len(exp_w) and len(exp_w) >= db.npk
            for i, (off, c, ln, p, j, st, flag, data) in enumerate(exp_w):
                w = r.wires[i]
                assert (int(w["out_off"]), int(w["counter"]), int(w["len"]), int(w["packet"]), int(w["segment"]),
                        int(w["reserved"])) == (off, c, ln, p, j, flag), i
                assert int(r.wire_status[i]) == st, i
                assert r.wire_bytes(i) == data, (i, p, j)
            assert r.tunnels["message_counter"].tolist() == exp_ctr
    finally:
        for k in held:
            k.close()


def test_coalesce_workspace_grows_under_a_queued_batch(fresh):
    """64 packets on stream A, then 1500 on stream B: past the 1024-packet floor."""
    import torch

    dev = torch.device("cuda", fresh.device)
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    runs = []
    for seed, n in ((61, 64), (62, 1500)):
        packets = K.random_batch(seed, n)
        plain, arena = K.stage(packets)
        cap = K.default_cap(packets)
        model = CM.coalesce(packets, K.BOTH, cap, n)
        bufs = dict(plain=up(plain), inp=up(arena), out=torch.zeros(cap + 64, dtype=torch.uint8, device=dev),
                    writes=torch.zeros((n + 1) * L.TUN_WRITE_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                    nw=torch.full((1,), -5, dtype=torch.int32, device=dev),
                    pw=torch.full((n,), -7, dtype=torch.int32, device=dev),
                    ps=torch.full((n,), -7, dtype=torch.int32, device=dev))
        runs.append((n, cap, model, bufs))
    streams = _two_streams()
    for (n, cap, _, b), s in zip(runs, streams):
        rc = L.lib().neb_rx_coalesce_batch(fresh.handle, p(b["plain"]), n, p(b["inp"]), p(b["out"]), cap, p(b["writes"]),
                                           n, p(b["nw"]), p(b["pw"]), p(b["ps"]), K.BOTH, C.c_void_p(s.cuda_stream))
        L.check(rc, "neb_rx_coalesce_batch")
    for s in streams:
        s.synchronize()
    for n, cap, model, b in runs:
        nw = int(b["nw"].item())
        assert 0 <= nw <= n
        w = b["writes"].cpu().numpy().view(L.TUN_WRITE_DTYPE)
        K.assert_equal_model(model, (w[:nw], b["out"].cpu().numpy(), b["pw"].cpu().numpy().view(np.uint32),
                                     b["ps"].cpu().numpy()), f"n {n}")


def _relay_batch(oracle_mod, alg, rng, in_keys, n, ntun):
    """n Message/Relay packets of the inbound tunnels in counter order, every 13th forged, routed over
    ntun target tunnels -> [(bytes, inbound tunnel)], routes"""
    ctr = [2] * len(in_keys)
    pkts, routes = [], []
    for i in range(n):
        t = i % len(in_keys)
        ctr[t] += 1
        inner = bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 90)))
        pkt = bytearray(RM.seal_relay(oracle_mod, alg, in_keys[t], 0x1000 + t, ctr[t], inner))
        if i % 13 == 7:
            pkt[-1] ^= 0x40
        pkts.append((bytes(pkt), t))
        routes.append((i % ntun, 0xA000 + i % ntun))
    return pkts, routes


def test_relay_workspace_grows_under_a_queued_forward(fresh, oracle_mod):
    """64 packets over 2 target tunnels on stream A, then 1500 over 80 on stream B, through one window
    set: past the forward workspace's 1024-packet and 64-tunnel floors. The receive half ends with its
    stream synchronized; the forward half of the first batch is what may still be queued."""
    import replay_oracle as R
    import torch

    from nebula_amd.connection_state import DeviceWindows
    from nebula_amd.inside import TX_TUNNEL_DTYPE
    from nebula_amd.relay import relay_forward_batch_device

    alg, window_len, slot = L.ALG_AESGCM, 1024, 160
    rng = random.Random(71)
    dev = torch.device("cuda", fresh.device)
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)  # noqa: E731
    dw = DeviceWindows(fresh, fresh.max_keys, window_len)
    nodes, runs = [], []
    try:
        for n, nin, ntun in ((64, 2, 2), (1500, 4, 80)):  # each batch has inbound tunnels of its own
            in_keys, tun_keys = _keys(rng, nin), _keys(rng, ntun)
            node = _Node(fresh, alg, in_keys, tun_keys)
            nodes.append(node)
            pkts, routes = _relay_batch(oracle_mod, alg, rng, in_keys, n, ntun)
            arena, packets = _lay_out(pkts, slot)
            counters = [10 + 1000 * t for t in range(ntun)]
            exp = RM.forward(oracle_mod, R, alg, in_keys, arena, packets, routes, list(zip(counters, tun_keys)),
                             window_len)
            wins = node.windows(window_len)
            for c, w in zip(node.cin, wins):
                dw.load(c.key_id, w)
            d = dict(pk=up(node.rx_packets(packets)), rt=up(np.array(routes, dtype=L.RELAY_ROUTE_DTYPE)),
                     tun=up(node.tunnels(counters)), arena=up(arena),
                     st=torch.full((n,), -1, dtype=torch.int32, device=dev),
                     fwd=torch.full((n,), -1, dtype=torch.int32, device=dev))
            runs.append((node, wins, exp, d))
        streams = _two_streams()
        for (_, _, _, d), s in zip(runs, streams):
            relay_forward_batch_device(fresh, alg, dw, d["pk"], d["rt"], d["tun"], d["arena"], d["st"], d["fwd"],
                                       L.KEYS_MIXED, stream=s.cuda_stream)
        for s in streams:
            s.synchronize()
        for node, wins, (exp_status, exp_fwd, exp_arena, owins, exp_ctr), d in runs:
            assert d["st"].cpu().numpy().tolist() == exp_status
            assert d["fwd"].cpu().numpy().tolist() == exp_fwd
            assert {R.OK, RM.NOT_FORWARDED} <= set(exp_fwd) and R.AUTH_FAILED in exp_status
            assert np.array_equal(d["arena"].cpu().numpy(), exp_arena)
            assert [int(c) for c in d["tun"].cpu().numpy().view(TX_TUNNEL_DTYPE)["message_counter"]] == exp_ctr
            for t, (c, w) in enumerate(zip(node.cin, wins)):
                dw.store(c.key_id, w)
                o = owins[t]
                assert (w.current, w.lost, w.dupe, w.out_of_window) == (o.current, o.lost, o.dupe, o.out_of_window)
    finally:
        dw.destroy()
        for node in nodes:
            node.close()


def test_scheduler_workspace_rebuilt_under_a_queued_batch(fresh, oracle_mod, knobs):
    """Mixed-key AES-GCM neb_seal_batch: 512 packets of 64 B over 64 keys on stream A with the tile
    threshold at its default, then 2048 such packets on stream B after KNOB_TILE_BINS_FROM = 1024: the
    scheduler workspace is rebuilt with the tile arrays while the first batch may still be queued."""
    from nebula_amd import workload as W
    from nebula_amd.batch import DeviceBatch, install_keys

    alg = L.ALG_AESGCM
    b1 = W.make_batch(alg, 512, 64, sizes=(64,), name="ws small")
    b2 = W.make_batch(alg, 2048, 64, sizes=(64,), name="ws tiles")
    assert np.array_equal(b1.keys, b2.keys)
    ciphers = install_keys(fresh, b1)
    try:
        runs = []
        for b in (b1, b2):
            ref = b.arena.copy()
            assert (oracle_mod.batch(alg, 0, b.keys, b.desc, ref) == 0).all()
            runs.append((DeviceBatch(fresh, b, ciphers), ref))
        assert all(db.key_hint == L.KEYS_MIXED for db, _ in runs)
        sa, sb = _two_streams()
        runs[0][0].seal(sa.cuda_stream)
        knobs(L.KNOB_TILE_BINS_FROM, 1024)
        runs[1][0].seal(sb.cuda_stream)
        sa.synchronize()
        sb.synchronize()
        for db, ref in runs:
            assert (db.status_host() == 0).all()
            assert np.array_equal(db.arena_host(), ref)
    finally:
        for c in ciphers:
            c.destroy()
