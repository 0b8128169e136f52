"""GPU: neb_rx_resolve_batch — the hostmap's index lookups for a whole receive batch on the device
— against the host form and the dict model (tests/resolve_ref.py) on the cases of
tests/resolve_cases.py; in front of the three receive calls; and what a resolve sees while the
table is updated on another stream or rebuilds itself."""
import ctypes as C
import random

import numpy as np
import pytest

import relay_forward_ref as RF
import resolve_cases as RC
import resolve_ref as M
import rx_via_ref as RV
from nebula_amd import _lib as L
from nebula_amd.hostmap import IndexTable

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


def _dev(engine):
    import torch

    return torch.device("cuda", engine.device)


def _up(engine, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev(engine))


def _down(t, dtype):
    return t.cpu().numpy().view(dtype).copy()


def _outputs(engine, n, fill=0xEE):
    import torch

    return (torch.full((n * 8,), fill, dtype=torch.uint8, device=_dev(engine)),
            torch.full((n * 8,), fill, dtype=torch.uint8, device=_dev(engine)))


def _assert_equal(case, model, n, pk, route, via, with_src=True):
    keys, lens, routes, vias = RC.expected(model, case, n, with_src)
    m = len(case.packets)
    assert pk["key_id"].tolist() == keys
    assert pk["len"].tolist() == lens
    assert pk["off"].tolist() == [case.packets[i % m][0] for i in range(n)]
    if route is not None:
        assert [tuple(r) for r in route.tolist()] == routes
    if via is not None:
        assert [tuple(v) for v in via.tolist()] == vias


@pytest.mark.parametrize("capacity", [8, 4096])
def test_device_equals_host_equals_model(engine, capacity):
    import torch

    case = RC.build(capacity, filler=1000 if capacity > 8 else 0)
    with IndexTable(engine, capacity) as t:
        RC.load(t, case)
        d_arena = _up(engine, case.arena)
        for n in SIZES:
            pk, src = RC.packet_array(case, n)
            host_pk = pk.copy()
            h_route, h_via = t.resolve_host(host_pk, case.arena.copy(), src)
            d_pk, d_src = _up(engine, pk), _up(engine, src)
            d_route, d_via = _outputs(engine, n)
            t.resolve_device(d_pk, d_arena, d_src, d_route, d_via)
            torch.cuda.synchronize()
            got_pk, got_route, got_via = _down(d_pk, L.RX_PACKET_DTYPE), _down(d_route, L.RELAY_ROUTE_DTYPE), _down(d_via, L.RX_VIA_DTYPE)
            _assert_equal(case, case.model, n, got_pk, got_route, got_via)
            assert got_pk.tobytes() == host_pk.tobytes() and got_route.tobytes() == h_route.tobytes()
            assert got_via.tobytes() == h_via.tobytes()
        assert np.array_equal(d_arena.cpu().numpy(), case.arena)  # the arena is only read
        # the /0 prefix, on the device too
        t.set_own_networks(RC.NETS_ZERO)
        zero = case.model.copy()
        zero.set_own_networks(RC.NETS_ZERO)
        pk, src = RC.packet_array(case, 257)
        d_pk, d_src = _up(engine, pk), _up(engine, src)
        d_route, d_via = _outputs(engine, 257)
        t.resolve_device(d_pk, d_arena, d_src, d_route, d_via)
        torch.cuda.synchronize()
        _assert_equal(case, zero, 257, _down(d_pk, L.RX_PACKET_DTYPE), _down(d_route, L.RELAY_ROUTE_DTYPE), _down(d_via, L.RX_VIA_DTYPE))


def test_null_arrays_and_empty_batch(engine):
    import torch

    case = RC.build(8)
    n = 257
    with IndexTable(engine, 8) as t:
        RC.load(t, case)
        d_arena = _up(engine, case.arena)
        pk, src = RC.packet_array(case, n)
        for drop in ("src", "route", "via"):
            d_pk, d_src = _up(engine, pk), _up(engine, src)
            d_route, d_via = _outputs(engine, n)
            t.resolve_device(d_pk, d_arena, None if drop == "src" else d_src, None if drop == "route" else d_route,
                             None if drop == "via" else d_via)
            torch.cuda.synchronize()
            route, via = _down(d_route, L.RELAY_ROUTE_DTYPE), _down(d_via, L.RX_VIA_DTYPE)
            _assert_equal(case, case.model, n, _down(d_pk, L.RX_PACKET_DTYPE), None if drop == "route" else route,
                          None if drop == "via" else via, with_src=drop != "src")
            if drop == "route":
                assert (d_route.cpu().numpy() == 0xEE).all()  # not written
            if drop == "via":
                assert (d_via.cpu().numpy() == 0xEE).all()
        lib = L.lib()
        d_pk = _up(engine, pk)
        before = d_pk.cpu().numpy().copy()
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        assert lib.neb_rx_resolve_batch(engine.handle, t.handle, p(d_pk), None, 0, p(d_arena), None, None, None) == L.OK
        assert lib.neb_rx_resolve_batch(engine.handle, t.handle, None, None, 0, None, None, None, None) == L.OK
        assert lib.neb_rx_resolve_batch(engine.handle, t.handle, None, None, 1, p(d_arena), None, None, None) == L.ERR_INVALID
        assert lib.neb_rx_resolve_batch(engine.handle, t.handle, p(d_pk), None, 1, None, None, None, None) == L.ERR_INVALID
        assert lib.neb_rx_resolve_batch(engine.handle, None, p(d_pk), None, 1, p(d_arena), None, None, None) == L.ERR_INVALID
        with IndexTable(None, 8) as host_only:
            assert lib.neb_rx_resolve_batch(engine.handle, host_only.handle, p(d_pk), None, 1, p(d_arena), None, None,
                                            None) == L.ERR_INVALID
        torch.cuda.synchronize()
        assert np.array_equal(d_pk.cpu().numpy(), before)


def test_one_update_larger_than_the_staging(engine):
    """9000 puts in one call go to the device in three launches through the two staging buffers
    (the third waits for the first); then 5000 deletions and 5000 replaces in one call."""
    import torch

    n = 9000
    rng = np.random.default_rng(9)
    index = rng.permutation(1 << 24)[:n].astype(np.uint32)
    rows = np.zeros(n, L.INDEX_ENTRY_DTYPE)
    rows["index"], rows["key_id"], rows["tunnel"] = index, np.arange(n) + 1, M.RELAY_NONE
    arena = np.zeros((n, 16), np.uint8)
    arena[:, 0] = 0x11
    arena[:, 4:8] = index.astype(">u4").reshape(-1, 1).view(np.uint8)
    pk = np.zeros(n, L.RX_PACKET_DTYPE)
    pk["off"], pk["len"] = np.arange(n) * 16, 16
    with IndexTable(engine, n) as t:
        t.update([], rows)
        d_arena, d_pk = _up(engine, arena), _up(engine, pk)
        t.resolve_device(d_pk, d_arena)
        torch.cuda.synchronize()
        assert np.array_equal(_down(d_pk, L.RX_PACKET_DTYPE)["key_id"], rows["key_id"])
        again = rows[4000:].copy()
        again["key_id"] += 100000
        t.update([(M.TUNNEL, int(i)) for i in index[:5000]], again)
        t.resolve_device(d_pk, d_arena)
        torch.cuda.synchronize()
        want = np.concatenate([np.full(4000, M.MIXED, np.uint32), again["key_id"]])
        assert np.array_equal(_down(d_pk, L.RX_PACKET_DTYPE)["key_id"], want) and t.count() == 5000


# ---- in front of the receive calls ----------------------------------------------------------------


def _windows_state(engine, dw, key_ids, window_len):
    from nebula_amd.connection_state import Bits

    out = []
    for k in key_ids:
        w = Bits(window_len)
        dw.store(k, w)
        out.append((w.current, w.lost, w.dupe, w.out_of_window, tuple(w.snapshot())))
        w.destroy()
    return out


@pytest.mark.parametrize("alg", [L.ALG_AESGCM, L.ALG_CHACHAPOLY])
def test_resolve_in_front_of_the_receive_calls(engine, oracle_mod, alg):
    """300 packets of a node behind relays that also forwards (8 tunnels, 2 relay indexes; the mix
    of tests/rx_via_ref.py, and relay packets of tests/relay_forward_ref.py). Each receive call on
    the arrays the device resolve filled gives, byte for byte, what it gives on arrays filled from
    the dict model: statuses, arena, windows, tunnel counters."""
    import torch

    from nebula_amd.connection_state import Bits, DeviceWindows, rx_open_wire_batch_device
    from nebula_amd.inside import TX_TUNNEL_DTYPE
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly
    from nebula_amd.relay import relay_forward_batch_device, rx_open_via_batch_device

    rng = random.Random(300 + alg)
    keys, pkts, _ = RV.random_batch(oracle_mod, alg, rng, 279, nrelay=2, ndirect=3, ntarget=3)
    for i in range(20):  # through the second relay index, longer inner packets
        inner = RF.seal_message(oracle_mod, alg, keys[5 + i % 3], 0x105 + i % 3, 5000 + i, bytes([i]) * (200 + 37 * i))
        pkts.insert(rng.randrange(len(pkts)), (RF.seal_relay(oracle_mod, alg, keys[1], 0x101, 9000 + i, inner), 1))
    pkts.insert(100, (RF.seal_message(oracle_mod, alg, keys[2], 0x999, 3, b"a tunnel we do not know"), None))
    n, slot, window_len = len(pkts), 1024, 256
    assert n == 300 and len(keys) == 8
    arena, packets = RV.lay_out(pkts, slot)
    cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
    ciphers = [cf.Cipher(engine, keys[t]) for t in range(8)]
    kid = [c.key_id for c in ciphers]
    try:
        # relay index 0x100 is a TerminalType relay (we are its target), 0x101 forwards to tunnel 1
        rows = [(M.TUNNEL, 0x100 + t, kid[t], 0, M.RELAY_NONE, 0) for t in range(8)]
        rows += [(M.RELAY, 0x100, kid[0], M.VIA_TERMINAL, M.RELAY_NONE, 0), (M.RELAY, 0x101, kid[1], 0, 1, 0x7788)]
        model = M.Model()
        model.update([], rows)
        raw = [(off, ln) for off, ln, _ in packets]
        m_keys, m_lens, m_routes, m_vias = model.resolve(arena, raw)
        assert sum(v[1] for v in m_vias) > 50 and sum(r[0] != M.RELAY_NONE for r in m_routes) >= 20
        assert m_keys[100] == M.MIXED and {kid[t] for t in range(5)} <= set(m_keys)
        pk_model = np.array([(off, ln, k) for (off, _), ln, k in zip(raw, m_lens, m_keys)], dtype=L.RX_PACKET_DTYPE)
        pk_blank = pk_model.copy()
        pk_blank["key_id"] = 0x0BAD0BAD
        tun = np.zeros(2, TX_TUNNEL_DTYPE)
        tun[0], tun[1] = (10, kid[6], 0x6000), (20, kid[7], 0x6001)
        count = max(kid) + 1
        zeros = lambda: torch.full((n,), -1, dtype=torch.int32, device=_dev(engine))  # noqa: E731

        def run(call, resolved):
            """One receive call on fresh windows, arena and tunnels -> everything it leaves behind."""
            dw = DeviceWindows(engine, count, window_len)
            try:
                for k in kid:
                    w = Bits(window_len)
                    dw.load(k, w)
                    w.destroy()
                d_arena, d_tun = _up(engine, arena), _up(engine, tun)
                if resolved:
                    with IndexTable(engine, 16) as t:
                        t.update([], rows)
                        d_pk = _up(engine, pk_blank)
                        d_route, d_via = _outputs(engine, n)
                        t.resolve_device(d_pk, d_arena, None, d_route, d_via)  # the call follows on the same stream
                        out = receive(call, dw, d_pk, d_route, d_via, d_arena, d_tun)
                else:
                    d_pk = _up(engine, pk_model)
                    d_route = _up(engine, np.array(m_routes, dtype=L.RELAY_ROUTE_DTYPE))
                    d_via = _up(engine, np.array(m_vias, dtype=L.RX_VIA_DTYPE))
                    out = receive(call, dw, d_pk, d_route, d_via, d_arena, d_tun)
                return out + (d_arena.cpu().numpy().tobytes(), d_tun.cpu().numpy().tobytes(), d_pk.cpu().numpy().tobytes(),
                              _windows_state(engine, dw, kid, window_len))
            finally:
                dw.destroy()

        def receive(call, dw, d_pk, d_route, d_via, d_arena, d_tun):
            d_st, d_st2 = zeros(), zeros()
            if call == "wire":
                rx_open_wire_batch_device(engine, alg, dw, d_pk, d_arena, d_st)
            elif call == "forward":
                relay_forward_batch_device(engine, alg, dw, d_pk, d_route, d_tun, d_arena, d_st, d_st2)
            else:
                d_inner = torch.zeros(n * 16, dtype=torch.uint8, device=_dev(engine))
                rx_open_via_batch_device(engine, alg, dw, d_pk, d_via, d_arena, d_st, d_inner, d_st2)
                torch.cuda.synchronize()
                return d_st.cpu().numpy().tolist(), d_st2.cpu().numpy().tolist(), d_inner.cpu().numpy().tobytes()
            torch.cuda.synchronize()
            return d_st.cpu().numpy().tolist(), d_st2.cpu().numpy().tolist(), b""

        for call in ("wire", "forward", "via"):
            want, got = run(call, False), run(call, True)
            names = ("status", "second status", "inner records", "arena", "tunnels", "packet records", "windows")
            for name, w, g in zip(names, want, got):
                assert w == g, f"{call}: {name} differ"
            assert want[0].count(0) > 150  # and the batch did real work
            if call == "forward":
                assert want[1].count(0) >= 20 and want[4] != tun.tobytes()
            if call == "via":
                assert want[1].count(0) > 50
    finally:
        for c in ciphers:
            c.destroy()


# ---- visibility -------------------------------------------------------------------------------------


def _headers(rows_outer, inner=None):
    """One packet per row: the outer header names the row's key; inner: a second header behind it."""
    out = bytearray()
    for k, (space, index) in enumerate(rows_outer):
        out += RC.header(1, 1, space, index)
        out += RC.header(1, 1, inner[k][0], inner[k][1]) if inner else bytes(16)
        out += bytes(16)
    return np.frombuffer(bytes(out), np.uint8).copy()


def test_steady_keys_never_miss_while_another_stream_updates(engine):
    """4096 steady entries; 64 churn keys put and deleted by 50 updates on stream A while 50 resolves
    of 4096 packets run on stream B. Every packet's outer header names a steady key; the odd ones
    are terminal relay packets whose inner header names a churn key. Whatever the interleaving, a
    steady key resolves to its record, a churn key to its record or to a miss."""
    import torch

    rng = random.Random(4096)
    steady = {}
    while len(steady) < 4096:
        k = len(steady)
        space = k & 1
        steady[(space, rng.getrandbits(32))] = (k + 1, M.VIA_TERMINAL if space else 0, M.RELAY_NONE if k % 4 != 3 else k, k * 3 if k % 4 == 3 else 0)
    churn = {}
    while len(churn) < 64:
        key = (M.TUNNEL, rng.getrandbits(32))
        if key not in steady:
            churn[key] = (50000 + len(churn), 0, M.RELAY_NONE, 0)
    skeys, ckeys = list(steady), list(churn)
    arena = _headers(skeys, [ckeys[i % 64] for i in range(4096)])
    pk = np.zeros(4096, L.RX_PACKET_DTYPE)
    pk["off"], pk["len"], pk["key_id"] = np.arange(4096) * 48, 48, 0x0BAD0BAD
    a, b = torch.cuda.Stream(_dev(engine)), torch.cuda.Stream(_dev(engine))
    with IndexTable(engine, 4096 + 64) as t:
        t.update([], [k + v for k, v in steady.items()], stream=a.cuda_stream)
        a.synchronize()
        d_arena = _up(engine, arena)
        outs = [(_up(engine, pk),) + _outputs(engine, 4096) for _ in range(50)]
        torch.cuda.synchronize()  # the uploads; from here on only the two streams under test
        live = set()
        for d_pk, d_route, d_via in outs:
            flip = set(rng.sample(ckeys, 32))
            t.update([k for k in flip if k in live], [k + churn[k] for k in flip if k not in live], stream=a.cuda_stream)
            live ^= flip
            t.resolve_device(d_pk, d_arena, None, d_route, d_via, stream=b.cuda_stream)
        a.synchronize()
        b.synchronize()
        want_key = np.array([steady[k][0] for k in skeys], np.uint32)
        want_route = np.array([(steady[k][2], steady[k][3]) if steady[k][2] != M.RELAY_NONE and k[0] else (M.RELAY_NONE, 0)
                               for k in skeys], dtype=L.RELAY_ROUTE_DTYPE)
        terminal = np.array([k[0] == M.RELAY for k in skeys])
        inner_key = np.array([churn[ckeys[i % 64]][0] for i in range(4096)], np.uint32)
        seen_hit = seen_miss = 0
        for d_pk, d_route, d_via in outs:
            got, route, via = _down(d_pk, L.RX_PACKET_DTYPE), _down(d_route, L.RELAY_ROUTE_DTYPE), _down(d_via, L.RX_VIA_DTYPE)
            assert np.array_equal(got["key_id"], want_key)  # no steady key ever misses
            assert route.tobytes() == want_route.tobytes()
            assert np.array_equal(via["flags"], terminal.astype(np.uint32))
            hit, miss = via["key_id"] == inner_key, via["key_id"] == M.MIXED
            assert (miss[~terminal]).all() and (hit | miss)[terminal].all()
            seen_hit += int(hit[terminal].sum())
            seen_miss += int(miss[terminal].sum())
        assert seen_hit and seen_miss
        # afterwards, on either stream, the table is the final state
        d_pk = _up(engine, pk)
        d_route, d_via = _outputs(engine, 4096)
        torch.cuda.current_stream().synchronize()
        t.resolve_device(d_pk, d_arena, None, d_route, d_via, stream=b.cuda_stream)
        b.synchronize()
        via = _down(d_via, L.RX_VIA_DTYPE)
        final = np.array([churn[ckeys[i % 64]][0] if ckeys[i % 64] in live else M.MIXED for i in range(4096)], np.uint32)
        assert np.array_equal(via["key_id"][terminal], final[terminal])
        assert t.count() == 4096 + len(live)


def test_rebuild_under_load(engine):
    """Twice: 8 resolves queued, a rebuild forced by updates that replace and delete records, 8
    more resolves; every output equals the model's for the table as it was when the resolve was
    enqueued. The second rebuild goes back into the image the very first resolves read."""
    import torch

    rng = random.Random(77)
    cap = 64
    m = M.Model()
    keys = []
    while len(keys) < 40:
        k = (rng.randrange(2), rng.getrandbits(32))
        if k not in keys:
            keys.append(k)
    absent = [(M.TUNNEL, 12345), (M.RELAY, 12345)]
    arena = _headers(keys + absent, [keys[(i * 7) % 40] for i in range(42)])
    packets = [(48 * i, 48) for i in range(42)]
    pk = np.zeros(42, L.RX_PACKET_DTYPE)
    pk["off"], pk["len"], pk["key_id"] = np.arange(42) * 48, 48, 0x0BAD0BAD

    def record(k, version):
        return (k[0], k[1], version * 100 + keys.index(k), (version + keys.index(k)) % 2 if k[0] else 0,
                (M.RELAY_NONE if (version + keys.index(k)) % 3 else version) if k[0] else M.RELAY_NONE, version)

    s = torch.cuda.Stream(_dev(engine))
    hot = keys[0]
    with IndexTable(engine, cap) as t:
        d_arena = _up(engine, arena)
        first = [record(k, 0) for k in keys[:32]]
        t.update([], first, stream=s.cuda_stream)
        m.update([], first)
        queued = []

        def resolve():
            d_pk = _up(engine, pk)
            d_route, d_via = _outputs(engine, 42)
            torch.cuda.current_stream().synchronize()
            t.resolve_device(d_pk, d_arena, None, d_route, d_via, stream=s.cuda_stream)
            queued.append((m.resolve(arena, packets), d_pk, d_route, d_via))

        version, rebuilds = 0, 0
        for _ in range(2):
            for _ in range(8):
                resolve()
            last = t.probe(*hot)[2]
            for _ in range(12):  # each update takes 33 slots of 256; the rebuild comes past 192
                version += 1
                gone = [k for k in rng.sample(keys[1:], 6) if k in m.entries]
                put = [record(hot, version)] + [record(k, version) for k in rng.sample(keys[1:], 32) if k not in gone]
                t.update(gone, put, stream=s.cuda_stream)
                m.update(gone, put)
                probes = t.probe(*hot)[2]
                if probes < last:  # the hot key's chain only shrinks in a rebuild
                    rebuilds += 1
                    break
                last = probes
            for _ in range(8):
                resolve()
        assert rebuilds == 2
        s.synchronize()
        assert len(queued) == 32
        for (keys_w, lens_w, routes_w, vias_w), d_pk, d_route, d_via in queued:
            got = _down(d_pk, L.RX_PACKET_DTYPE)
            assert got["key_id"].tolist() == keys_w and got["len"].tolist() == lens_w
            assert [tuple(r) for r in _down(d_route, L.RELAY_ROUTE_DTYPE).tolist()] == routes_w
            assert [tuple(v) for v in _down(d_via, L.RX_VIA_DTYPE).tolist()] == vias_w
        assert t.count() == len(m.entries)
