"""GPU: neb_rx_recv_plan against the model (tests/recv_plan_ref.py): every directed case of
tests/recv_plan_cases.py and a seeded random set, all six outputs byte for byte with everything beyond
max_packets / nentries untouched, with control buffers and with seg_size, and once with the optional
outputs NULL; one engine's workspace reused at alternating sizes and the same plan twice in a row; and
the plan in front of neb_rx_resolve_batch and neb_rx_open_wire_batch on one stream."""
import ctypes as C
import random

import numpy as np
import pytest

import recv_plan_cases as RC
import recv_plan_ref as M
import relay_forward_ref as RF
import resolve_ref as RM
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

SLACK = 3


def _dev(engine):
    import torch

    return torch.device("cuda", engine.device)


def _up(engine, a, pad=0):
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([raw, np.full(pad, 0xEE, np.uint8)])).to(_dev(engine))


class _Inputs:
    """A batch's entries and control slots on the device (8 spare bytes behind each: never empty)."""

    def __init__(self, engine, b):
        en, ctrl = RC.arrays(b)
        self.b, self.n = b, len(en)
        self.d_en, self.d_ctrl = _up(engine, en, 8), _up(engine, ctrl, 8)


def _plan(engine, inp, use_ctrl, max_packets, optional=True):
    """The device form into FILL-initialised outputs with SLACK elements beyond each. Returns the raw
    output bytes by name and the counts."""
    import torch

    size = {"pk": max_packets, "src": max_packets, "pkt_entry": max_packets, "from": inp.n, "entry_first": inp.n}
    outs = {name: torch.full(((size[name] + SLACK) * item,), RC.FILL, dtype=torch.uint8, device=_dev(engine))
            for name, item in RC.OUT_ITEMS}
    cnt = torch.full((2,), -1, dtype=torch.int32, device=_dev(engine))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    opt = lambda t: p(t) if optional else None  # noqa: E731
    rc = L.lib().neb_rx_recv_plan(engine.handle, p(inp.d_en), inp.n, p(inp.d_ctrl) if use_ctrl else None, inp.b.ctrl_stride,
                                  int(inp.b.socket_v4), p(outs["pk"]), opt(outs["src"]), opt(outs["pkt_entry"]), max_packets,
                                  opt(outs["from"]), p(outs["entry_first"]), p(cnt),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, "neb_rx_recv_plan")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, cnt.cpu().numpy().view(np.uint32)


_WANT = {}


def _want(key, b, use_ctrl):
    """The model's outputs, computed once per (case, mode)."""
    if (key, use_ctrl) not in _WANT:
        p = M.listen_out(b, use_ctrl)
        _WANT[key, use_ctrl] = (p.max_packets, RC.plan_arrays(p, len(b.entries)))
    return _WANT[key, use_ctrl]


def _check(engine, key, b, inp=None, modes=((True, True), (False, True), (True, False))):
    inp = _Inputs(engine, b) if inp is None else inp
    for use_ctrl, optional in modes:
        mp, want = _want(key, b, use_ctrl)
        out, counts = _plan(engine, inp, use_ctrl, mp, optional)
        try:
            RC.compare(out, counts, want, SLACK, optional)
        except AssertionError as e:
            raise AssertionError(f"{key} (ctrl={use_ctrl}, optional outputs={optional}): {e}") from e
    return inp


DIRECTED = RC.directed()


@pytest.mark.parametrize("case", DIRECTED, ids=[c.name for c in DIRECTED])
def test_directed_case(engine, case):
    _check(engine, case.name, case.batch)


def test_random_batches(engine):
    for k, b in enumerate(RC.random_batches(4242, 60)):
        _check(engine, ("random", k), b, modes=((bool(k & 1), k % 4 != 0), (not k & 1, True)))


def test_workspace_reuse_and_the_same_plan_twice(engine):
    """Entry counts alternating around the workspace's sizes on one engine, each plan twice in a row."""
    by = {c.name: c for c in DIRECTED}
    names = ("entries_5000", "entries_255", "entries_70000", "entries_257", "entry_of_65535_middle", "entries_1", "entries_70000",
             "entries_256")
    inputs = {}
    for name in names:
        for _ in range(2):
            inputs[name] = _check(engine, name, by[name].batch, inputs.get(name), modes=((True, True),))


def test_argument_errors(engine):
    import torch

    z = torch.zeros(4096, dtype=torch.uint8, device=_dev(engine))
    at = lambda k: C.c_void_p(z.data_ptr() + k)  # noqa: E731
    p, c, q, lib, h = at(0), at(512), at(4), L.lib(), engine.handle
    call = lambda **o: lib.neb_rx_recv_plan(*{**dict(e=h, en=p, n=2, ctrl=c, stride=64, v4=1, pk=at(1024), src=at(1536),  # noqa: E731
                                                     pe=at(2048), mp=8, frm=at(2560), first=at(3072), counts=at(3584), s=None),
                                              **o}.values())
    assert call() == L.OK
    for over in (dict(e=None), dict(en=None), dict(pk=None), dict(first=None), dict(counts=None), dict(n=1 << 31), dict(mp=1 << 31),
                 dict(stride=0), dict(stride=12), dict(stride=1032), dict(en=q), dict(ctrl=q)):
        assert call(**over) == L.ERR_INVALID, over
    assert call(en=None, n=0) == L.OK and call(ctrl=None, stride=0) == L.OK and call(src=None, pe=None, frm=None) == L.OK
    assert call(mp=0) == L.OK and call(en=None, n=0, mp=0) == L.OK
    torch.cuda.synchronize()


def _windows_state(engine, dw, key_ids, window_len):
    from nebula_amd.connection_state import Bits

    out = []
    for k in key_ids:
        w = Bits(window_len)
        dw.store(k, w)
        out.append((w.current, w.lost, w.dupe, w.out_of_window, tuple(w.snapshot())))
        w.destroy()
    return out


@pytest.mark.parametrize("alg", [L.ALG_AESGCM])
def test_plan_in_front_of_resolve_and_open_on_one_stream(engine, oracle_mod, alg):
    """Sealed wire packets of six tunnels, each from its own source, packed as UDP_GRO would: runs of
    equal-length packets of one source back to back in one buffer, a shorter one last, singletons
    among them. Plan, resolve and open over max_packets = total + 37 on one stream with nothing in
    between, against resolve and open over hand-built per-packet descriptors."""
    import torch

    from nebula_amd.connection_state import Bits, DeviceWindows, rx_open_wire_batch_device
    from nebula_amd.hostmap import IndexTable
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly
    from nebula_amd.outside import recv_plan_device

    rng = random.Random(1364)
    ntun, window_len, stride = 6, 256, 32
    keys = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(ntun)]
    names = [RC.sockaddr6(RC.mapped(f"10.7.0.{t + 1}"), 4000 + t) if t % 2 else RC.sockaddr6(f"2001:db8::{t + 1}", 4000 + t)
             for t in range(ntun)]
    counter = [10] * ntun
    entries, hand, chunks, at = [], [], [], 0
    while len(hand) < 300:
        t = rng.randrange(ntun)
        nseg = rng.choice([1, 1, 2, 3, 8, 21])
        plen = rng.choice([1, 64, 500, 1316])
        seg = 16 + plen + 16
        sizes = [plen] * nseg
        if nseg > 1 and rng.random() < 0.5:
            sizes[-1] = rng.randrange(0, plen)  # a shorter last segment
        buf = b""
        for k, sz in enumerate(sizes):
            replay = len(hand) % 29 == 28
            c = counter[t] - 1 if replay else counter[t]
            counter[t] += 0 if replay else 1
            pkt = RF.seal_message(oracle_mod, alg, keys[t], 0x200 + (t if len(hand) % 41 != 40 else 99), c, bytes([len(hand) & 255]) * sz)
            hand.append((at + len(buf), len(pkt), t))
            buf += pkt
        entries.append(RC.entry(len(buf), seg if nseg > 1 else 0, off=at, name=names[t], decoy=-1))
        chunks.append(buf)
        at += (len(buf) + 63) & ~63
    at += 64
    b = RC.batch(entries, socket_v4=False, ctrl_stride=stride, lay_out=False)
    total = len(hand)
    mp = total + 37
    arena = np.full(at, 0x5C, np.uint8)
    for e, buf in zip(entries, chunks):
        arena[e.off:e.off + len(buf)] = np.frombuffer(buf, np.uint8)
    plan = M.listen_out(b, True)
    assert plan.npackets == total and plan.pk == [(o, n) for o, n, _ in hand] and max(plan.count) >= 8
    assert any(c > 2 and RC.lens(plan, j)[-1] < RC.lens(plan, j)[0] for j, c in enumerate(plan.count))  # shorter last segments
    assert plan.count.count(1) > 10
    hand_pk = np.array([(o, n, 0x0BAD0BAD) for o, n, _ in hand], dtype=L.RX_PACKET_DTYPE)
    hand_src = RC.plan_arrays(plan, len(entries))[1][:total]

    cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
    ciphers = [cf.Cipher(engine, k) for k in keys]
    kid = [c.key_id for c in ciphers]
    rows = [(RM.TUNNEL, 0x200 + t, kid[t], 0, RM.RELAY_NONE, 0) for t in range(ntun)]

    def run(planned):
        dw = DeviceWindows(engine, max(kid) + 1, window_len)
        try:
            for k in kid:
                w = Bits(window_len)
                dw.load(k, w)
                w.destroy()
            with IndexTable(engine, 16) as tab:
                tab.update([], rows)
                tab.set_own_networks(["10.7.0.2/32"])  # tunnel 1's source is one of our own addresses
                d_arena = _up(engine, arena)
                n = mp if planned else total
                d_st = torch.full((n,), -1, dtype=torch.int32, device=_dev(engine))
                if planned:
                    en, ctrl = RC.arrays(b)
                    d_en, d_ctrl = _up(engine, en), _up(engine, ctrl)
                    d_pk = torch.full((mp * 16,), RC.FILL, dtype=torch.uint8, device=_dev(engine))
                    d_src = torch.full((mp * 20,), RC.FILL, dtype=torch.uint8, device=_dev(engine))
                    d_first = torch.zeros(len(en), dtype=torch.int32, device=_dev(engine))
                    d_cnt = torch.zeros(2, dtype=torch.int32, device=_dev(engine))
                    torch.cuda.synchronize()  # the uploads; from here on one stream, nothing in between
                    recv_plan_device(engine, d_en, False, d_pk, d_first, d_cnt, d_src=d_src, d_ctrl=d_ctrl, ctrl_stride=stride)
                else:
                    d_pk, d_src = _up(engine, hand_pk), _up(engine, hand_src)
                    d_cnt = None
                tab.resolve_device(d_pk, d_arena, d_src)
                rx_open_wire_batch_device(engine, alg, dw, d_pk, d_arena, d_st)
                torch.cuda.synchronize()
                return (d_st.cpu().numpy(), d_pk.cpu().numpy().view(L.RX_PACKET_DTYPE), d_arena.cpu().numpy(),
                        _windows_state(engine, dw, kid, window_len), None if d_cnt is None else d_cnt.cpu().tolist())
        finally:
            dw.destroy()

    try:
        want, got = run(False), run(True)
    finally:
        for c in ciphers:
            c.destroy()
    assert got[4] == [total, len(entries)]
    assert got[0][:total].tolist() == want[0].tolist(), "statuses differ"
    assert got[1][:total].tobytes() == want[1].tobytes(), "packet records differ"
    assert got[2].tobytes() == want[2].tobytes(), "arenas differ"
    assert got[3] == want[3], "windows differ"
    # the padding: refused by the gate, its records as the plan wrote them
    assert got[0][total:].tolist() == [L.STATUS_INVALID] * 37
    assert got[1][total:].tolist() == [(0, 0, L.KEYS_MIXED)] * 37
    # and the batch did real work: opened packets, replays, an unknown index, own-source drops
    st = want[0].tolist()
    assert st.count(L.STATUS_OK) > 150 and len(set(st)) >= 4
    assert (want[1]["len"] & L.RX_OWN_SOURCE).any() and L.KEYS_MIXED in want[1]["key_id"].tolist()
    assert want[2].tobytes() != arena.tobytes() and (want[2][-64:] == 0x5C).all()
