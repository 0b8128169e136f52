"""GPU: the directed receive-coalescer cases (tests/coalesce_edge_cases.py; what they reach is checked
on the CPU in tests/test_coalesce_edge_cases.py) through neb_rx_coalesce_batch, bit-exact against the
sequential model (coalesce_ref.py), with test_gpu_rx_coalesce.py's canaries and read-only check:
every case twice in a row on the shared engine, sizes alternating large and small; the gather cases
and the reference's scenarios again with both arenas off a 16-byte boundary; the runs that need every
pointer-jumping round under capacity cuts that fall inside the run; the flow sort's lane bit with one
hash group per lane; and wire packets whose epochs and counters differ in high bits, end to end."""
import functools
import random

import numpy as np
import pytest

import coalesce_cases as K
import coalesce_edge_cases as E
import coalesce_ref as M
from nebula_amd import _lib as L
from test_gpu_rx_coalesce import run_device

pytestmark = pytest.mark.gpu
CASES = E.all_cases()
BY_NAME = {c[0]: c for c in CASES + K.named_cases()}
SHIFTS = [(1, 0), (0, 1), (8, 15), (15, 7)]


@functools.lru_cache(maxsize=None)
def model(name):
    _, packets, lanes = BY_NAME[name]
    return M.coalesce(packets, lanes)


def same(a, b):
    """Two results of run_device are identical: writes, the whole output arena, per-packet results."""
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_twice(engine, name, **kw):
    _, packets, lanes = BY_NAME[name]
    first = run_device(engine, packets, lanes, stage=K.stage_padded, **kw)
    K.assert_equal_model(model(name), first, name)
    assert same(first, run_device(engine, packets, lanes, stage=K.stage_padded, **kw)), f"{name}: second run differs"


@pytest.mark.parametrize("fam", ["sort", "jump", "gather", "rule"])
def test_directed_cases_twice_large_small_large(engine, fam):
    order = E.large_small_large(E.family(CASES, fam))
    sizes = [len(c[1]) for c in order]
    assert sizes[0] > sizes[1] < sizes[2]
    for name, _, _ in order:
        check_twice(engine, name)


@pytest.mark.parametrize("shift", SHIFTS, ids=lambda s: f"in{s[0]}_out{s[1]}")
def test_arenas_off_a_16_byte_boundary(engine, shift):
    """d_in and d_out as views `shift` bytes off a 16-byte boundary: out_off stays a 16-aligned offset,
    the addresses are not aligned (the header allows it). Canaries on both sides of the output."""
    for name, _, _ in E.family(CASES, "gather") + K.named_cases():
        check_twice(engine, name, shift=shift)


def test_capacity_cuts_inside_a_run_that_needs_every_round(engine):
    """max_writes and out_cap fall inside the run: the seeds marked last are the ones cut off."""
    for name in ("jump_psh_257", "jump_udp_257", "jump_psh_1025", "jump_half_plus_one"):
        _, packets, lanes = BY_NAME[name]
        full = model(name)[0]
        run = [k for k, w in enumerate(full) if w["lane"] != M.LANE_PT and w["nseg"] == 1]
        assert len(run) > len(packets) // 2
        ends = [w["out_off"] + M.align16(w["len"]) for w in full]
        last = run[-1]
        for mw, cap in ((last, None), (last - 1, None), (run[len(run) // 2] + 1, None), (None, ends[last] - 1),
                        (None, ends[last - 1]), (None, ends[run[len(run) // 2]])):
            mw = len(packets) if mw is None else mw
            cap = K.default_cap(packets) if cap is None else cap
            want = M.coalesce(packets, lanes, cap, mw)
            assert 0 < len(want[0]) < len(full) and M.ST_NO_SPACE in want[2]
            got = run_device(engine, packets, lanes, cap, mw, stage=K.stage_padded)
            K.assert_equal_model(want, got, f"{name} max_writes {mw} out_cap {cap}")


def test_lane_bit_with_one_hash_group_per_lane(engine, knobs):
    """NEB_KNOB_COALESCE_HASH_BITS 0: only the lane bit of the flow sort's key keeps a TCP flow and a
    UDP flow with the same addresses and ports apart, and only co_flow_equal the two families."""
    for name in ("rule_tcp_udp_same_tuple", "rule_family_only"):
        check_twice(engine, name)
    knobs(L.KNOB_COALESCE_HASH_BITS, 0)
    for name in ("rule_tcp_udp_same_tuple", "rule_family_only", "rule_barrier_in_other_lane"):
        check_twice(engine, name)


def test_wire_to_tun_writes_with_64_bit_keys(engine, oracle_mod):
    """Three tunnels whose epochs (from the epoch table) differ in bit 63, 32 and below, each sealing
    counters 1 << i, i = 0..61 (below the receive's 2^62 threshold), arrive interleaved; one TCP flow
    runs over them in (epoch, counter) order, so the device's own plain records must sort on the high
    bits to give back its chains of 64."""
    import torch

    import relay_forward_ref as R
    from nebula_amd import outside as O
    from nebula_amd.connection_state import Bits, DeviceWindows
    from nebula_amd.noiseutil import CipherAESGCM

    alg = L.ALG_AESGCM
    r = random.Random(9)
    epochs = [(1 << 63) + 5, 1 << 32, 7]
    keys = [bytes(r.getrandbits(8) for _ in range(32)) for _ in epochs]
    ciphers = [CipherAESGCM.Cipher(engine, k) for k in keys]
    dw = None
    try:
        sent = sorted((epochs[t], 1 << i, t) for t in range(3) for i in range(62))
        rank = {(t, c): j for j, (_, c, t) in enumerate(sent)}  # the flow's segment j is sent j-th
        arena, pk, expect = bytearray(b"\0" * 5), [], []
        for i in range(62):  # arrival: the tunnels in turn, each tunnel's counters ascending
            for t in range(3):
                c = 1 << i
                data = K.seg(rank[t, c], size=100)
                wire = R.seal_message(oracle_mod, alg, keys[t], 0x200 + t, c, data)
                pk.append((len(arena), len(wire), ciphers[t].key_id))
                expect.append(dict(data=data, epoch=epochs[t], counter=c, flags=0))
                arena += wire
        n = len(pk)
        epoch = np.zeros(max(c.key_id for c in ciphers) + 1, np.uint64)
        for t, c in enumerate(ciphers):
            epoch[c.key_id] = epochs[t]
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
        d_out = torch.full((cap + 64,), 0xC7, dtype=torch.uint8, device=dev)
        d_writes = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        d_nw = torch.zeros(1, dtype=torch.int32, device=dev)
        d_pw = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ps = torch.zeros(n, dtype=torch.int32, device=dev)
        O.receive(engine, alg, dw, d_pk, d_arena, d_st, d_epoch.view(torch.int64), d_plain, d_out[:cap], d_writes,
                  d_nw, d_pw, d_ps)
        torch.cuda.synchronize(dev)
        assert not d_st.cpu().numpy().any(), "every packet opens"
        plain = d_plain.cpu().numpy().view(L.PLAIN_PACKET_DTYPE)
        assert [(int(g["epoch"]), int(g["counter"]), int(g["len"])) for g in plain] == \
            [(e["epoch"], e["counter"], len(e["data"])) for e in expect]
        want = M.coalesce(expect, K.BOTH, cap, n)
        assert [(w["nseg"], w["first"]) for w in want[0]] == [(64, 2), (64, 7), (58, 12)]
        out = d_out.cpu().numpy()
        assert (out[cap:] == 0xC7).all(), "wrote past out_cap"
        writes = d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:int(d_nw.item())]
        K.assert_equal_model(want, (writes, out, d_pw.cpu().numpy().view(np.uint32), d_ps.cpu().numpy()), "wire")
    finally:
        if dw is not None:
            dw.destroy()
        for c in ciphers:
            c.destroy()
