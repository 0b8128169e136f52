"""GPU: neb_tx_send_plan against the sequential model (tests/send_plan_ref.py): every directed case
of tests/send_plan_cases.py, all six outputs; exact and slack capacities with everything beyond the
counts untouched; wire counts around the block size and across scan tiles; one engine's workspace
reused at alternating sizes; *d_nwires = 0 over a non-empty array; the plan queued straight behind
neb_tx_seal_via_batch on one stream; and C2's TX shape with offsets past 2^32."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import send_plan_cases as SC
import send_plan_ref as M
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _device_plan(engine, b, max_wires=None, nwires=None):
    """The device form over the batch's arrays; the outputs hold max_wires elements filled with FILL.
    Returns the raw output bytes and the two counts."""
    import torch

    dev = torch.device("cuda", engine.device)
    wires, st, packets, via, remote = SC.arrays(b)
    n = len(wires)
    max_wires = n if max_wires is None else max_wires
    up = lambda a, pad=0: torch.from_numpy(np.concatenate([a.view(np.uint8).reshape(-1), np.full(pad, 0xEE, np.uint8)]).copy()).to(dev)  # noqa: E731
    d_w = up(wires, (max_wires - n) * 32 + 32)   # the slots past n hold garbage; never empty
    d_st = up(st, (max_wires - n) * 4 + 4)
    d_pk = up(packets, 32)
    d_rm = up(remote, 20)
    d_via = None if via is None else up(via)
    d_n = torch.tensor([n if nwires is None else nwires], dtype=torch.int32, device=dev)
    outs = [torch.full((max(max_wires, 1) * sz,), FILL, dtype=torch.uint8, device=dev) for sz in (16, 16, 4, 4)]
    cnt = torch.full((2,), -1, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_tx_send_plan(engine.handle, p(d_w), p(d_st), p(d_n), max_wires, p(d_pk), len(packets),
                                  None if d_via is None else p(d_via), p(d_rm), len(remote), int(b.socket_v4), b.max_segments,
                                  b.chunk_packets, p(outs[0]), C.c_void_p(cnt.data_ptr()), p(outs[1]),
                                  C.c_void_p(cnt.data_ptr() + 4), p(outs[2]), p(outs[3]),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, "neb_tx_send_plan")
    torch.cuda.synchronize()
    ni, ne = (int(x) for x in cnt.cpu())
    return [o.cpu().numpy() for o in outs], ni, ne


def _check(engine, b, slack=0, want=None):
    want = M.sequential(b) if want is None else want
    n = len(b.lens)
    outs, ni, ne = _device_plan(engine, b, max_wires=n + slack)
    if n + slack == 0:  # max_wires == 0: NEB_OK, nothing written, the counts included
        assert (ni, ne) == (-1, -1)
        return want
    w_iov, w_ent, w_we, w_st = SC.plan_arrays(want)
    assert (ni, ne) == (len(w_iov), len(w_ent))
    for name, got, w, item, cnt in (("send_status", outs[3], w_st, 4, n), ("wire_entry", outs[2], w_we, 4, n),
                                    ("iov", outs[0], w_iov, 16, ni), ("entries", outs[1], w_ent, 16, ne)):
        assert got[:cnt * item].tobytes() == w.tobytes(), name
        assert (got[cnt * item:] == FILL).all(), name  # beyond the counts: untouched
    return want


DIRECTED = SC.directed()


@pytest.mark.parametrize("slack", [0, 5])
def test_directed_cases(engine, slack):
    for case in DIRECTED:
        try:
            _check(engine, case.batch, slack)
        except AssertionError as e:
            raise AssertionError(f"{case.name}: {e}") from e


def test_parity_chain(engine):
    """Every run's end decides the next run's start over 4097 wires: the composition's order and
    the carry between the scan's tiles."""
    full = _check(engine, SC.parity_chain(False))
    dropped = _check(engine, SC.parity_chain(True), slack=3)
    assert {full.iov[e[0]][2] for e in full.entries}.isdisjoint({dropped.iov[e[0]][2] for e in dropped.entries})


def test_random_batches(engine):
    for b in SC.random_batches(77, 60, nmax=70):
        _check(engine, b, slack=len(b.lens) % 3)


def test_sizes_and_workspace_reuse(engine):
    """255, 256, 257 and 4097 wires, twice in a row on one engine with the sizes alternating."""
    batches = {n: SC.sized(n, n) for n in (255, 256, 257, 4097)}
    want = {n: M.sequential(b) for n, b in batches.items()}
    for n in (4097, 255, 257, 256, 4097, 256, 255, 257):
        _check(engine, batches[n], slack=0 if n != 257 else 40, want=want[n])


def test_no_wires_on_a_non_empty_array(engine):
    b = SC.sized(300, 9)
    outs, ni, ne = _device_plan(engine, b, nwires=0)
    assert (ni, ne) == (0, 0) and all((o == FILL).all() for o in outs)
    # and a count below the array's: the plan of the first 100
    sub = M.Batch(lens=b.lens[:100], packet=b.packet[:100], flags=b.flags[:100], status=b.status[:100], pkt_tunnel=b.pkt_tunnel,
                  remote=b.remote, via=b.via, out_off=b.out_off[:100])
    want = SC.plan_arrays(M.sequential(sub))
    outs, ni, ne = _device_plan(engine, b, nwires=100)
    assert (ni, ne) == (len(want[0]), len(want[1]))
    assert outs[0][:ni * 16].tobytes() == want[0].tobytes() and outs[1][:ne * 16].tobytes() == want[1].tobytes()
    assert outs[2][:400].tobytes() == want[2].tobytes() and (outs[2][400:] == FILL).all()
    assert outs[3][:400].tobytes() == want[3].tobytes() and (outs[3][400:] == FILL).all()


def test_max_wires_zero_and_argument_errors(engine):
    lib = L.lib()
    assert lib.neb_tx_send_plan(engine.handle, None, None, None, 0, None, 0, None, None, 0, 1, 63, 128, None, None, None, None,
                                None, None, None) == L.ERR_INVALID  # the counts' pointers are required
    z = np.zeros(8, np.uint32)
    p = z.ctypes.data_as(C.c_void_p)
    assert lib.neb_tx_send_plan(engine.handle, None, None, p, 0, None, 0, None, None, 0, 1, 63, 128, None, p, None, p, None,
                                None, None) == L.OK
    assert lib.neb_tx_send_plan(engine.handle, None, None, p, 4, None, 0, None, None, 0, 1, 63, 128, None, p, None, p, None,
                                None, None) == L.ERR_INVALID


def test_plan_behind_the_seal_on_one_stream(engine):
    """64 TSO reads over 8 tunnels, two of them through one relay, one tunnel's counter running out:
    neb_tx_seal_via_batch, then the plan on the same stream with nothing between them."""
    import torch

    import segment_oracle as S
    from nebula_amd.inside import DeviceSendPlan, DeviceTxBatch
    from test_gpu_tx import _pk, _to_arrays, _tunnels
    from test_gpu_tx_via import _Keys
    from test_segment_oracle import build_tcpv4_super

    rng = random.Random(64)
    tun = _tunnels(rng, n=8, keyless=())
    tun[3]["counter"] = S.REJECT_AFTER - 7   # runs out inside its second read
    via = np.zeros(8, L.RELAY_ROUTE_DTYPE)
    via["tunnel"] = L.RELAY_NONE
    via[5] = (7, 0x7500)
    via[6] = (7, 0x7600)
    remote = [SC.v4(f"10.9.0.{t}") for t in range(8)]
    remote[5] = remote[6] = (0, b"\0" * 16, 0, 0)
    P = []
    for k in range(64):
        tcp, _, cs = build_tcpv4_super(4000 + 137 * (k % 9))
        P.append(_pk(tcp, [0, 5, 7, 6, 3, 1, 2, 4][k % 8] if k % 16 < 12 else 7 - (k % 2) * 2, 1, S.GSO_TCPV4, 1000, cs, 16))
    pk, arena = _to_arrays(P)
    K = _Keys(engine, L.ALG_AESGCM, tun)
    try:
        db = DeviceTxBatch(engine, L.ALG_AESGCM, K.tun, pk, arena, 1 << 20, 512, via=via)
        sp = DeviceSendPlan(db, SC.arrays(SC.batch([], remote=remote))[4], True, 63, 128)
        db.seal()
        sp.plan()
        torch.cuda.synchronize()
        r, got = db.result(), sp.result()
    finally:
        K.close()
    n = len(r.wires)
    assert n >= 64 * 4 and L.STATUS_EXHAUSTED in r.wire_status.tolist() and L.TX_WIRE_VIA in r.wires["reserved"].tolist()
    b = M.Batch(lens=r.wires["len"].tolist(), packet=r.wires["packet"].tolist(), flags=r.wires["reserved"].tolist(),
                status=r.wire_status.tolist(), pkt_tunnel=pk["tunnel"].tolist(), remote=remote, via=via["tunnel"].tolist(),
                out_off=r.wires["out_off"].tolist())
    want = M.sequential(b)
    w_iov, w_ent, w_we, w_st = SC.plan_arrays(want)
    assert got.send_status.tobytes() == w_st.tobytes() and got.wire_entry.tobytes() == w_we.tobytes()
    assert got.iov.tobytes() == w_iov.tobytes() and got.entries.tobytes() == w_ent.tobytes()
    assert M.NOT_SENT in want.send_status and max(e[1] for e in want.entries) >= 5
    assert any(e[3] == 7 and e[1] >= 2 for e in want.entries)  # runs to the relay's remote


def test_c2_shape_with_offsets_past_32_bits(engine):
    """65 520 wires (1456 reads of 45 segments) over 4096 tunnels, the slots laid out across 2^32."""
    nread, nseg = 1456, 45
    lens = ([1332] * (nseg - 1) + [700]) * nread
    base = (1 << 32) - 1344 * 1000
    remote = [SC.v4(f"10.{1 + t // 65536}.{(t >> 8) & 255}.{t & 255}") for t in range(4096)]
    b = M.Batch(lens=lens, packet=[i // nseg for i in range(nread * nseg)], flags=[0] * len(lens), status=[0] * len(lens),
                pkt_tunnel=[(7 * r) % 4096 for r in range(nread)], remote=remote, via=None,
                out_off=[base + 1344 * i for i in range(len(lens))])
    want = M.sequential(b)
    assert len(want.iov) == 65520 and want.iov[-1][0] > 1 << 32 and len(want.entries) > 1456
    outs, ni, ne = _device_plan(engine, b)
    w_iov, w_ent, w_we, w_st = SC.plan_arrays(want)
    assert (ni, ne) == (len(w_iov), len(w_ent)) and ni == 65520
    for got, w in zip(outs, (w_iov, w_ent, w_we, w_st)):
        assert hashlib.sha256(got[:w.nbytes].tobytes()).hexdigest() == hashlib.sha256(w.tobytes()).hexdigest()
