"""GPU: neb_tx_resolve_batch — newPacket, the own-address gates and the VPN address / route lookup
for a whole batch of TUN reads on the device — against the host form and the model
(tests/tx_resolve_ref.py) on the cases of tests/tx_resolve_cases.py; in front of the two TX seal
calls; and what a resolve sees while hosts are updated on another stream, routes are replaced from
another thread, or the table rebuilds itself."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import tx_resolve_cases as TC
import tx_resolve_ref as M
from nebula_amd import _lib as L
from nebula_amd.hostmap import TxTable
from nebula_amd.inside import TX_PACKET_DTYPE

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
FW = L.FW_PACKET_DTYPE.itemsize


def _dev(engine):
    import torch

    return torch.device("cuda", engine.device)


def _up(engine, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev(engine))


def _outputs(engine, n):
    import torch

    return (torch.full((n * FW,), 0xEE, dtype=torch.uint8, device=_dev(engine)),
            torch.full((n,), -7, dtype=torch.int32, device=_dev(engine)))


def _table(engine):
    return TxTable(engine, TC.HOSTS, TC.ROUTES, TC.GATEWAYS)


def test_device_equals_host_equals_model(engine):
    import torch

    case = TC.build()
    with _table(engine) as t:
        TC.load(t, case)
        d_in = _up(engine, case.arena)
        for n in SIZES:
            pk = TC.packet_array(case, n)
            tunnels, statuses, fwb = TC.expected(case.model, case, n)
            host_pk = pk.copy()
            h_fw, h_st = t.resolve_host(host_pk, case.arena)
            for with_fw in (True, False):
                d_pk = _up(engine, pk)
                d_fw, d_st = _outputs(engine, n)
                t.resolve_device(d_pk, d_in, d_fw if with_fw else None, d_st)
                torch.cuda.synchronize()
                got = d_pk.cpu().numpy().view(TX_PACKET_DTYPE)
                assert got["tunnel"].tolist() == tunnels == host_pk["tunnel"].tolist()
                assert d_st.cpu().numpy().tolist() == statuses == h_st.tolist()
                assert (got["in_off"] == pk["in_off"]).all() and (got["len"] == pk["len"]).all()
                if with_fw:
                    assert d_fw.cpu().numpy().tobytes() == fwb == h_fw.tobytes()
                else:
                    assert (d_fw.cpu().numpy() == 0xEE).all()  # not written
        assert np.array_equal(d_in.cpu().numpy(), case.arena)  # the input is only read
        # no status array; an empty batch; bad arguments
        lib = L.lib()
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        d_pk = _up(engine, TC.packet_array(case, 65))
        t.resolve_device(d_pk, d_in)
        torch.cuda.synchronize()
        assert d_pk.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"].tolist() == TC.expected(case.model, case, 65)[0]
        assert lib.neb_tx_resolve_batch(engine.handle, t.handle, None, 0, None, None, None, None) == L.OK
        assert lib.neb_tx_resolve_batch(engine.handle, t.handle, None, 1, p(d_in), None, None, None) == L.ERR_INVALID
        assert lib.neb_tx_resolve_batch(engine.handle, t.handle, p(d_pk), 1, None, None, None, None) == L.ERR_INVALID
        assert lib.neb_tx_resolve_batch(engine.handle, t.handle, p(d_pk), 1, p(d_in), C.c_void_p(d_in.data_ptr() + 8), None,
                                        None) == L.ERR_INVALID  # fw is 16-byte aligned
        with TxTable(None, 8) as host_only:
            assert lib.neb_tx_resolve_batch(engine.handle, host_only.handle, p(d_pk), 1, p(d_in), None, None, None) == L.ERR_INVALID


def _tx_batch(case):
    """A few dozen plain reads of the case set and two TSO reads, bound for hosts of the table."""
    from nebula_amd.inside import GSO_TCPV4, GSO_TCPV6
    from test_segment_oracle import build_tcpv4_super, build_tcpv6_super

    reads = [dict(data=bytes(p)) for _, p in case.items[:48]]
    tcp, _, cs = build_tcpv4_super(5000)
    tcp = bytearray(tcp)
    tcp[16:20] = M.ipaddress.ip_address("10.1.0.20").packed
    reads.insert(7, dict(data=bytes(tcp), vnet_flags=1, gso_type=GSO_TCPV4, gso_size=1448, csum_start=cs, csum_offset=16))
    tcp6, _, cs6 = build_tcpv6_super(3001)
    tcp6 = bytearray(tcp6)
    tcp6[24:40] = M.ipaddress.ip_address("fd00:1::20").packed
    reads.insert(30, dict(data=bytes(tcp6), vnet_flags=1, gso_type=GSO_TCPV6, gso_size=1000, csum_start=cs6, csum_offset=16))
    arena, pk = bytearray(), np.zeros(len(reads), TX_PACKET_DTYPE)
    for i, r in enumerate(reads):
        arena.extend(bytes(-len(arena) % 16 + (2 if i % 2 else 0)))  # 16-aligned, and 2 past it as behind a virtio header
        pk[i]["in_off"], pk[i]["len"] = len(arena), len(r["data"])
        for f in ("vnet_flags", "gso_type", "gso_size", "csum_start", "csum_offset"):
            pk[i][f] = r.get(f, 0)
        arena.extend(r["data"])
    arena.extend(bytes(64))
    model = [case.model.resolve(r["data"]) for r in reads]
    return pk, np.frombuffer(bytes(arena), np.uint8).copy(), model


@pytest.mark.parametrize("alg,via", [(L.ALG_AESGCM, False), (L.ALG_CHACHAPOLY, False), (L.ALG_AESGCM, True)])
def test_resolve_in_front_of_the_seal(engine, alg, via):
    """The seal on the tunnels the device resolve wrote gives, byte for byte, what it gives on
    tunnels filled from the model: wires, statuses, output bytes, tunnel counters."""
    import torch

    from nebula_amd.inside import TX_TUNNEL_DTYPE, DeviceTxBatch
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

    case = TC.build()
    rng = random.Random(40 + alg)
    pk, arena, model = _tx_batch(case)
    ntun = 20
    cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
    ciphers = [cf.Cipher(engine, bytes(rng.getrandbits(8) for _ in range(32))) for _ in range(ntun)]
    try:
        tun = np.zeros(ntun, TX_TUNNEL_DTYPE)
        for k, c in enumerate(ciphers):
            tun[k] = (100 * k + 1, c.key_id, 0xB000 + k)
        relay = None
        if via:  # tunnels 1 and 3 are reached through tunnel 4
            relay = np.array([(4, 0x7700 + k) if k in (1, 3) else (L.RELAY_NONE, 0) for k in range(ntun)], dtype=L.RELAY_ROUTE_DTYPE)
        pk_model, pk_blank = pk.copy(), pk.copy()
        pk_model["tunnel"] = [m[0] for m in model]
        pk_blank["tunnel"] = 0xEEEEEEEE
        results = []
        with _table(engine) as t:
            TC.load(t, case)
            for resolved in (False, True):
                db = DeviceTxBatch(engine, alg, tun, pk_blank if resolved else pk_model, arena, 1 << 18, 512, via=relay)
                d_fw, d_st = _outputs(engine, len(pk))
                torch.cuda.synchronize()
                if resolved:
                    t.resolve_device(db.packets, db.inp, d_fw, d_st)  # the seal follows on the same stream
                db.seal()
                torch.cuda.synchronize()
                r = db.result()
                results.append((r.wires.tobytes(), r.wire_status.tolist(), r.packet_status.tolist(), r.out.tobytes(),
                                r.tunnels.tobytes()))
                if resolved:
                    assert d_st.cpu().numpy().tolist() == [m[1] for m in model]
                    assert d_fw.cpu().numpy().tobytes() == b"".join(m[2] for m in model)
        for name, w, g in zip(("wires", "wire status", "packet status", "output", "tunnels"), *results):
            assert w == g, name
        pst = results[0][2]
        dropped = [i for i, m in enumerate(model) if m[1] != M.OK]
        # a dropped read falls out of the seal (BAD_KEY, or INVALID where the seal's own checks come first)
        assert dropped and all(pst[i] in (L.STATUS_BAD_KEY, L.STATUS_INVALID) for i in dropped)
        assert sum(pst[i] == L.STATUS_BAD_KEY for i in dropped) >= 5
        assert pst.count(L.STATUS_OK) >= 20 and len(results[0][1]) >= 20 + 4 + 4  # and the batch did real work
        assert results[0][4] != tun.tobytes()
    finally:
        for c in ciphers:
            c.destroy()


def _dst_batch(dsts):
    """One UDP read per destination, back to back."""
    reads = [TC.v6(d) if ":" in d else TC.v4(d) for d in dsts]
    arena = b"".join(reads)
    pk = np.zeros(len(dsts), TX_PACKET_DTYPE)
    at = 0
    for i, r in enumerate(reads):
        pk[i]["in_off"], pk[i]["len"] = at, len(r)
        at += len(r)
    pk["tunnel"] = 0xEEEEEEEE
    return pk, np.frombuffer(arena, np.uint8).copy()


def test_steady_hosts_never_miss_while_another_stream_updates(engine):
    """48 steady hosts; 16 churn addresses deleted, put and replaced by 40 updates on stream A while
    40 resolves run on stream B. A steady address resolves to its tunnel in every batch, a churn
    address to its old or its new tunnel or to NO_TUNNEL where it was deleted, and to nothing else."""
    import torch

    rng = random.Random(48)
    steady = [f"10.1.0.{k}" for k in range(20, 52)] + [f"fd00:1::{k:x}" for k in range(0x20, 0x30)]
    churn = [f"10.1.0.{k}" for k in range(100, 116)]
    dsts = steady + churn
    pk, arena = _dst_batch(dsts)
    a, b = torch.cuda.Stream(_dev(engine)), torch.cuda.Stream(_dev(engine))
    with _table(engine) as t:
        t.set_own(TC.OWN, True, True)
        t.update_hosts([], [(s, k) for k, s in enumerate(steady)], stream=a.cuda_stream)
        a.synchronize()
        d_in = _up(engine, arena)
        outs = [(_up(engine, pk),) + _outputs(engine, len(pk)) for _ in range(40)]
        torch.cuda.synchronize()
        state, allowed = {}, []
        for step, (d_pk, d_fw, d_st) in enumerate(outs):
            flip = rng.sample(churn, 8)
            dl = [c for c in flip if c in state and rng.random() < 0.5]
            pt = [(c, 1000 + step) for c in flip if c not in dl]
            before = dict(state)
            t.update_hosts(dl, pt, stream=a.cuda_stream)
            for c in dl:
                del state[c]
            state.update(pt)
            allowed.append(before)
            t.resolve_device(d_pk, d_in, d_fw, d_st, stream=b.cuda_stream)
        a.synchronize()
        b.synchronize()
        # B is not ordered against A: a batch may run before or after any of the updates
        history = allowed + [dict(state)]
        for step, (d_pk, d_fw, d_st) in enumerate(outs):
            got = d_pk.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"].tolist()
            st = d_st.cpu().numpy().tolist()
            assert got[:48] == list(range(48)) and st[:48] == [M.OK] * 48  # no steady address ever misses
            for k, c in enumerate(churn):
                may = {h.get(c, M.NO_TUNNEL_INDEX) for h in history}
                assert got[48 + k] in may, (step, c)
                assert st[48 + k] == (M.NO_TUNNEL if got[48 + k] == M.NO_TUNNEL_INDEX else M.OK)
        # afterwards, on either stream, the table is the final state
        d_pk = _up(engine, pk)
        torch.cuda.current_stream().synchronize()
        t.resolve_device(d_pk, d_in, stream=b.cuda_stream)
        b.synchronize()
        got = d_pk.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"].tolist()
        assert got[48:] == [state.get(c, M.NO_TUNNEL_INDEX) for c in churn]
        assert t.count() == (48 + len(state), 0)


def test_one_update_larger_than_the_staging(engine):
    """2 * 4096 + 1 puts in one call go to the device in three launches through the two staging
    buffers (the third waits for the first); then 4097 deletions and 4097 puts of other addresses in
    one call, two launches each. Neither call reaches the rebuild threshold (3/4 of 65536 slots).
    After each, one launch resolves all 8193 + 4097 addresses: device = host = model."""
    import torch

    first = [f"10.{64 + (k >> 16)}.{(k >> 8) & 255}.{k & 255}" for k in range(256, 256 + 8193)]
    others = [f"fd00:1::1:{k:x}" for k in range(1, 4098)]
    own = ("10.64.0.7/10", "fd00:1::7/64")
    pk, arena = _dst_batch(first + others)
    n = len(pk)
    model = M.Model()
    model.set_own(own)

    def check(t, d_in):
        d_pk = _up(engine, pk)
        d_fw, d_st = _outputs(engine, n)
        t.resolve_device(d_pk, d_in, d_fw, d_st)
        torch.cuda.synchronize()
        host_pk = pk.copy()
        h_fw, h_st = t.resolve_host(host_pk, arena)
        want = [model.resolve(arena[int(p["in_off"]):int(p["in_off"]) + int(p["len"])].tobytes()) for p in pk]
        got = d_pk.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"].tolist()
        assert got == host_pk["tunnel"].tolist() == [w[0] for w in want]
        assert d_st.cpu().numpy().tolist() == h_st.tolist() == [w[1] for w in want]
        assert d_fw.cpu().numpy().tobytes() == h_fw.tobytes() == b"".join(w[2] for w in want)
        return got

    with TxTable(engine, 16384) as t:
        t.set_own(own)
        d_in = _up(engine, arena)
        put = [(a, k + 1) for k, a in enumerate(first)]
        t.update_hosts([], put)
        model.update_hosts([], put)
        got = check(t, d_in)
        assert got == list(range(1, 8194)) + [M.NO_TUNNEL_INDEX] * 4097 and t.count() == (8193, 0)
        put = [(a, 100000 + k) for k, a in enumerate(others)]
        t.update_hosts(first[:4097], put)
        model.update_hosts(first[:4097], put)
        got = check(t, d_in)
        assert got == [M.NO_TUNNEL_INDEX] * 4097 + list(range(4098, 8194)) + list(range(100000, 104097))
        assert t.count() == (8193, 0)
        assert t.probe(first[0])[0] is False and t.probe(others[0])[0] is True


def test_routes_replaced_from_another_thread_under_load(engine):
    """set_routes from a host thread while resolves are enqueued: every batch equals the model under
    the old set or under the new set, entirely; the first batch after the call returns sees the new
    set."""
    import torch

    case = TC.build()
    n = len(case.items)
    pk = TC.packet_array(case, n)
    model_b = case.model.copy()
    model_b.set_routes(TC.ROUTES_B)
    want = {"a": TC.expected(case.model, case, n), "b": TC.expected(model_b, case, n)}
    assert want["a"][0] != want["b"][0]
    s, u = torch.cuda.Stream(_dev(engine)), torch.cuda.Stream(_dev(engine))
    with _table(engine) as t:
        TC.load(t, case)
        d_in = _up(engine, case.arena)
        outs = [(_up(engine, pk),) + _outputs(engine, n) for _ in range(64)]
        torch.cuda.synchronize()
        now = "a"
        for round_ in range(4):
            nxt = "b" if now == "a" else "a"
            started = threading.Event()

            def replace():
                started.set()
                t.set_routes(TC.ROUTES_B if nxt == "b" else TC.ROUTES_A, stream=u.cuda_stream)

            th = threading.Thread(target=replace)
            batch = outs[16 * round_:16 * round_ + 16]
            th.start()
            started.wait()
            for d_pk, d_fw, d_st in batch[:15]:
                t.resolve_device(d_pk, d_in, d_fw, d_st, stream=s.cuda_stream)
            th.join()
            t.resolve_device(*batch[15][:1], d_in, *batch[15][1:], stream=s.cuda_stream)  # after the call returned
            s.synchronize()
            for k, (d_pk, d_fw, d_st) in enumerate(batch):
                got = (d_pk.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"].tolist(), d_st.cpu().numpy().tolist(),
                       d_fw.cpu().numpy().tobytes())
                assert got in ((want[nxt],) if k == 15 else (want[now], want[nxt])), (round_, k)
            now = nxt


def test_rebuild_under_load(engine):
    """Twice: 8 resolves queued, a rebuild forced by host updates that replace and delete, 8 more
    resolves, all on one stream; every output equals the model's for the table as it was when the
    resolve was enqueued. The second rebuild goes back into the image the first resolves read."""
    import torch

    case = TC.build()
    n = len(case.items)
    pk = TC.packet_array(case, n)
    rng = random.Random(7)
    churn = [f"10.1.0.{k}" for k in range(100, 130)]
    hot = "10.1.0.20"
    s = torch.cuda.Stream(_dev(engine))
    with _table(engine) as t:
        TC.load(t, case)
        model = case.model.copy()
        d_in = _up(engine, case.arena)
        queued = []

        def resolve():
            d_pk = _up(engine, pk)
            d_fw, d_st = _outputs(engine, n)
            torch.cuda.current_stream().synchronize()
            t.resolve_device(d_pk, d_in, d_fw, d_st, stream=s.cuda_stream)
            queued.append((TC.expected(model, case, n), d_pk, d_fw, d_st))

        rebuilds = 0
        for _ in range(2):
            for _ in range(8):
                resolve()
            last = t.probe(hot)[2]
            for step in range(40):  # each update takes 25 slots of 512; the rebuild comes past 384
                gone = rng.sample(churn, 5)
                put = [(hot, 1)] + [(c, rng.randrange(TC.NTUNNELS)) for c in rng.sample(churn, 24) if c not in gone]
                t.update_hosts(gone, put, stream=s.cuda_stream)
                model.update_hosts(gone, put)
                probes = t.probe(hot)[2]
                if probes < last:  # the hot address's chain only shrinks in a rebuild
                    rebuilds += 1
                    break
                last = probes
            for _ in range(8):
                resolve()
        assert rebuilds == 2
        s.synchronize()
        assert len(queued) == 32
        for (tunnels, statuses, fwb), d_pk, d_fw, d_st in queued:
            assert d_pk.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"].tolist() == tunnels
            assert d_st.cpu().numpy().tolist() == statuses
            assert d_fw.cpu().numpy().tobytes() == fwb
        assert t.count() == (len(model.hosts), len(TC.ROUTES_A))
