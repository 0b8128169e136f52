"""GPU: neb_rx_coalesce_batch / neb_rx_plain_from_wire (nebula_amd/csrc/coalesce.hip) against the
sequential model of the reference's MultiCoalescer (coalesce_ref.py; tests/test_rx_coalesce.py ties
the host form to the same model on the CPU): every named scenario, the randomised mix below and
above one scan tile, one long flow (the chain search across workgroups), the segment cap, one-packet
flows, forced hash collisions, capacity cuts, and wire packets to TUN writes end to end."""
import ctypes as C
import random

import numpy as np
import pytest

import coalesce_cases as K
import coalesce_ref as M
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu
CANARY = 0xC7


def run_device(engine, packets, lanes=K.BOTH, out_cap=None, max_writes=None, stage=K.stage, shift=(0, 0)):
    """stage: how the packets are laid out in the input arena. shift: d_in and d_out are views that
    start this many bytes off a 16-byte boundary (out_off stays a 16-aligned offset into d_out)."""
    import torch

    dev = torch.device("cuda", engine.device)
    plain, arena = stage(packets)
    n = len(packets)
    cap = K.default_cap(packets) if out_cap is None else out_cap
    mw = n if max_writes is None else max_writes
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_plain = up(plain)
    in_buf = torch.zeros(shift[0] + arena.size, dtype=torch.uint8, device=dev)
    d_in = in_buf[shift[0]:]
    d_in.copy_(up(arena))
    front = 64 + shift[1]
    out_buf = torch.full((front + cap + 64,), CANARY, dtype=torch.uint8, device=dev)
    d_out = out_buf[front:]
    assert (d_in.data_ptr() % 16, d_out.data_ptr() % 16) == shift
    d_writes = torch.zeros((mw + 1) * L.TUN_WRITE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_nw = torch.full((1,), -5, dtype=torch.int32, device=dev)
    d_pw = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_ps = torch.full((n,), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_coalesce_batch(engine.handle, p(d_plain), n, p(d_in), p(d_out), cap, p(d_writes), mw, p(d_nw),
                                       p(d_pw), p(d_ps), lanes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, "neb_rx_coalesce_batch")
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    assert (out[cap:] == CANARY).all(), "wrote past out_cap"
    assert (out_buf[:front].cpu().numpy() == CANARY).all(), "wrote in front of the output arena"
    assert (d_in.cpu().numpy() == arena).all(), "the input arena is read-only"
    nw = int(d_nw.item())
    assert 0 <= nw <= mw
    w = d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)
    assert not w[nw:]["len"].any(), "wrote past nwrites"
    return w[:nw], out, d_pw.cpu().numpy().view(np.uint32), d_ps.cpu().numpy()


def check(engine, packets, lanes=K.BOTH, out_cap=None, max_writes=None, what=""):
    cap = K.default_cap(packets) if out_cap is None else out_cap
    mw = len(packets) if max_writes is None else max_writes
    model = M.coalesce(packets, lanes, cap, mw)
    K.assert_equal_model(model, run_device(engine, packets, lanes, cap, mw), what)
    return model


def test_named_cases(engine):
    for name, packets, lanes in K.named_cases():
        check(engine, packets, lanes, what=name)


@pytest.mark.parametrize("n", [3000, 20000])
def test_randomised_mix(engine, n):
    packets = K.random_batch(21 + n, n)
    model = check(engine, packets, what=f"n {n}")
    assert sum(w["nseg"] >= 2 for w in model[0]) >= 50


def test_one_long_flow_byte_cap(engine):
    """20 000 x 1300 B of one TCP flow: 400 chains of 50 segments in one run of linked packets."""
    packets = K.seq_([K.seg(i, size=1300, ident=i & 0xFFFF) for i in range(20000)])
    model = check(engine, packets)
    assert [w["nseg"] for w in model[0]] == [50] * 400


def test_one_flow_segment_cap(engine):
    packets = K.seq_([K.seg(i, size=100, ident=i) for i in range(1000)])
    model = check(engine, packets)
    assert [w["nseg"] for w in model[0]] == [64] * 15 + [40]


def test_many_one_packet_flows(engine):
    packets = K.seq_([K.seg(0, size=200, sport=1 + i % 60000, src=M.ip4(f"10.2.{i // 60000}.1")) if i % 3 else
                      K.dgram(0, size=200, sport=1 + i) for i in range(5000)])
    model = check(engine, packets)
    assert len(model[0]) == 5000


def test_hash_collisions_do_not_decide_equality(engine, knobs):
    packets = K.random_batch(31, 3000)
    knobs(L.KNOB_COALESCE_HASH_BITS, 2)
    check(engine, packets, what="2 hash bits")
    knobs(L.KNOB_COALESCE_HASH_BITS, 0)
    check(engine, packets[:600], what="0 hash bits")


def test_capacity_cuts(engine):
    packets = next(p for n, p, _ in K.named_cases() if n == "multi_restores_transmission_order") + \
        K.seq_([K.seg(i, sport=1500 + i) for i in range(6)], epoch=5)
    full = M.coalesce(packets)
    nw = len(full[0])
    for mw in (0, 1, 4, nw - 1, nw, nw + 3):
        m = check(engine, packets, max_writes=mw, what=f"max_writes {mw}")
        assert len(m[0]) == min(mw, nw)
    ends = [w["out_off"] + M.align16(w["len"]) for w in full[0]]
    for cap in (0, 15, ends[0] - 1, ends[0], ends[3], ends[4] - 16, ends[-1] - 1, ends[-1]):
        m = check(engine, packets, out_cap=cap, what=f"out_cap {cap}")
        assert len(m[0]) == sum(e <= cap for e in ends)


def test_multicoalescer_device_form(engine):
    from nebula_amd import MultiCoalescer

    m = MultiCoalescer(engine=engine)
    for i in (2, 0, 1):
        m.Commit(K.seg(i), 1, 10 + i)
    m.Commit(K.dgram(0), 1, 5, (M.UDP, False, 20))
    ws = m.Flush()
    assert [(w.lane, w.nseg, w.flags) for w in ws] == [(0, 3, 1), (1, 1, 2)]
    assert ws[1].data == K.dgram(0)


def test_wire_to_tun_writes_end_to_end(engine, oracle_mod):
    """The oracle seals 2000 messages of 3 tunnels (TCP / UDP flows, a few reordered, some control and
    test messages, forged tags, one replay); the device opens them, turns them into commit records
    and coalesces: the writes equal the model's over the plaintexts the model says are committed."""
    import torch

    import relay_forward_ref as R
    from nebula_amd import outside as O
    from nebula_amd.connection_state import Bits, DeviceWindows
    from nebula_amd.noiseutil import CipherAESGCM

    alg = L.ALG_AESGCM
    r = random.Random(5)
    keys = [bytes(r.getrandbits(8) for _ in range(32)) for _ in range(3)]
    ciphers = [CipherAESGCM.Cipher(engine, k) for k in keys]
    dw = None
    try:
        inner = K.random_batch(77, 2000)
        ctr = [10, 10, 10]
        arena, pk, expect = bytearray(b"\0" * 7), [], []
        for i, p in enumerate(inner):
            t = i * 3 // len(inner) if i % 5 else r.randrange(3)
            ctr[t] += 1
            typ, sub = (1, 0) if i % 97 else r.choice([(5, 0), (6, 0), (1, 1)])
            wire = bytearray(R.seal_message(oracle_mod, alg, keys[t], 0x100 + t, ctr[t], p["data"], typ, sub))
            forged = i % 131 == 7
            if forged:
                wire[-1] ^= 1
            pk.append((len(arena), len(wire), ciphers[t].key_id))
            committed = not forged and (typ, sub) == (1, 0)
            expect.append(dict(data=p["data"] if committed else b"", epoch=40 + t, counter=ctr[t],
                               flags=0 if committed else M.PLAIN_SKIP))
            arena += wire
        pk.append(pk[3])  # a replay
        expect.append(dict(data=b"", epoch=0, counter=0, flags=M.PLAIN_SKIP))
        n = len(pk)
        nslots = max(c.key_id for c in ciphers) + 1
        epoch = np.zeros(nslots, np.uint64)
        for t, c in enumerate(ciphers):
            epoch[c.key_id] = 40 + t
        pkt = np.array(pk, L.RX_PACKET_DTYPE)
        dev = torch.device("cuda", engine.device)
        dw = DeviceWindows(engine, engine.max_keys, 1024)
        for c in ciphers:
            w = Bits(1024)
            dw.load(c.key_id, w)
            w.destroy()
        cap = sum(M.align16(len(p["data"])) for p in expect)
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_pk, d_arena, d_epoch = up(pkt), up(np.frombuffer(bytes(arena), np.uint8)), up(epoch)
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_plain = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
        d_writes = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_nw = torch.zeros(1, dtype=torch.int32, device=dev)
        d_pw = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ps = torch.zeros(n, dtype=torch.int32, device=dev)
        O.receive(engine, alg, dw, d_pk, d_arena, d_st, d_epoch.view(torch.int64), d_plain, d_out[:cap], d_writes,
                  d_nw, d_pw, d_ps)
        torch.cuda.synchronize(dev)
        st = d_st.cpu().numpy()
        assert int(st[-1]) == L.STATUS_REPLAY and (st != 0).sum() >= 10
        plain = d_plain.cpu().numpy().view(L.PLAIN_PACKET_DTYPE)
        # the device's commit records equal the host twin's and the rule's
        host = O.plain_from_wire_host(pkt, st, epoch, np.frombuffer(bytes(arena), np.uint8))
        assert plain.tobytes() == host.tobytes()
        for i, (g, e) in enumerate(zip(plain, expect)):
            assert bool(g["flags"] & L.PLAIN_SKIP) == bool(e["flags"]), i
            if not e["flags"]:
                assert (int(g["off"]), int(g["len"]), int(g["epoch"]), int(g["counter"])) == \
                    (pk[i][0] + 16, len(e["data"]), e["epoch"], e["counter"])
        model = M.coalesce(expect, K.BOTH, cap, n)
        writes = d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:int(d_nw.item())]
        K.assert_equal_model(model, (writes, d_out.cpu().numpy(), d_pw.cpu().numpy().view(np.uint32),
                                     d_ps.cpu().numpy()), "end to end")
        assert sum(w["nseg"] >= 2 for w in model[0]) >= 20
    finally:
        if dw is not None:
            dw.destroy()
        for c in ciphers:
            c.destroy()
