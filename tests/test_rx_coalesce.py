"""CPU: neb_rx_coalesce_batch_host / neb_rx_plain_from_wire_host (nebula_amd/csrc/coalesce.cpp over
coalesce_core.hpp) against the sequential model of the reference's MultiCoalescer (coalesce_ref.py):
one named case per scenario of the reference's coalescer tests, the checksum seeds, the newPacket
derivation, the round trip through the TX segmentation oracle, a randomised mix, capacity cuts and
the wire-to-plain rule. No GPU is used."""
import ctypes as C
import struct

import numpy as np
import pytest

import coalesce_cases as K
import coalesce_ref as M
import segment_oracle as S
from nebula_amd import _lib as L
from nebula_amd import outside as O

CASES = K.named_cases()


def run_host(packets, lanes=K.BOTH, out_cap=None, max_writes=None):
    plain, arena = K.stage(packets)
    before = arena.copy()
    cap = K.default_cap(packets) if out_cap is None else out_cap
    got = O.coalesce_batch_host(plain, arena, lanes, cap, len(packets) if max_writes is None else max_writes)
    assert (arena == before).all(), "the input arena is read-only"
    return got


def check(packets, lanes=K.BOTH, out_cap=None, max_writes=None, what=""):
    cap = K.default_cap(packets) if out_cap is None else out_cap
    mw = len(packets) if max_writes is None else max_writes
    model = M.coalesce(packets, lanes, cap, mw)
    K.assert_equal_model(model, run_host(packets, lanes, cap, mw), what)
    return model


@pytest.mark.parametrize("name,packets,lanes", CASES, ids=[c[0] for c in CASES])
def test_named_case(name, packets, lanes):
    check(packets, lanes, what=name)


def _shape(name):
    """[(lane, nseg)] of the model's writes: pins what each scenario is about, independent of the host form."""
    packets, lanes = next((p, l) for n, p, l in CASES if n == name)
    return [(w["lane"], w["nseg"]) for w in M.coalesce(packets, lanes)[0]]


def test_model_shapes_of_the_named_cases():
    """The model itself does what the reference's tests assert (so agreeing with it means something)."""
    T, U, PT = M.LANE_TCP, M.LANE_UDP, M.LANE_PT
    assert _shape("tcp_seed_then_flush_alone") == [(T, 1)]
    assert _shape("tcp_pure_ack_does_not_seal") == [(T, 3), (T, 1)]
    assert _shape("tcp_fin_seals_flow") == [(T, 2), (T, 1), (T, 2)]
    assert _shape("tcp_adjacent_coalesce") == [(T, 4)]
    assert _shape("tcp_seq_gap") == [(T, 2), (T, 2)]
    assert _shape("tcp_ece_mismatch") == [(T, 1), (T, 2), (T, 1)]
    assert _shape("tcp_ect0_vs_ect1") == [(T, 1), (T, 2)]
    assert _shape("tcp_dscp_mismatch") == [(T, 1), (T, 2)]
    assert _shape("tcp_short_last_closes") == [(T, 3), (T, 2)]
    assert _shape("tcp_psh_finalises_and_propagates") == [(T, 3), (T, 2)]
    assert _shape("tcp_psh_on_seed") == [(T, 1), (T, 2)]
    assert _shape("tcp_different_flow") == [(T, 1)] * 3
    assert _shape("tcp_ip_options") == [(T, 2), (T, 1), (T, 2)]
    assert _shape("tcp_cap_64_segments") == [(T, 64), (T, 6)]
    assert _shape("tcp_cap_65535_bytes") == [(T, 50), (T, 10)]
    assert _shape("tcp_interleaved_flows_creation_order") == [(T, 4)] * 3
    assert _shape("tcp_v6_ece_flow") == [(T, 3)]
    assert _shape("tcp_v6_differing_ecn") == [(T, 1), (T, 2)]
    assert _shape("tcp_df_clear_sequential_ids") == [(T, 4)]
    assert _shape("tcp_df_clear_id_gap") == [(T, 2), (T, 2)]
    assert _shape("tcp_df_set_random_ids") == [(T, 4)]
    assert _shape("tcp_seq_wraparound") == [(T, 3)]
    assert _shape("tcp_unparseable_seals_all") == [(T, 1), (T, 1), (T, 1), (T, 2), (T, 2)]
    assert _shape("udp_equal_sized") == [(U, 4)]
    assert _shape("udp_short_last") == [(U, 3), (U, 2)]
    assert _shape("udp_larger_than_seed_reseeds") == [(U, 1), (U, 2)]
    assert _shape("udp_max_segments") == [(U, 64), (U, 6)]
    assert _shape("udp_zero_length_seals_keeps_order") == [(U, 2), (U, 1), (U, 2)]
    assert _shape("udp_v4_fragment_and_options") == [(U, 2), (U, 1), (U, 1), (U, 1), (U, 2)]
    assert _shape("udp_v6") == [(U, 3)]
    assert _shape("multi_routes_by_proto") == [(T, 3), (U, 3), (PT, 1), (PT, 1), (PT, 1)]
    assert _shape("multi_restores_transmission_order") == [(T, 4), (T, 4), (U, 4)]
    assert _shape("multi_epoch_orders_across_rehandshake") == [(T, 6)]
    assert _shape("multi_lanes_without_udp") == [(T, 4), (T, 4)] + [(PT, 1)] * 4
    assert _shape("multi_lanes_none_still_sorts") == [(PT, 1)] * 12
    assert _shape("multi_v6_fragment_stays_in_lane") == [(T, 2), (T, 1), (T, 2), (U, 1), (U, 1), (U, 1)]


def test_psh_propagates_and_seed_header_is_patched():
    packets = next(p for n, p, _ in CASES if n == "tcp_psh_finalises_and_propagates")
    writes, out, _, _ = run_host(packets)
    w = writes[0]
    o = int(w["out_off"])
    assert out[o + 20 + 13] & M.PSH and int(w["vnet_flags"]) == M.F_NEEDS_CSUM and int(w["gso_type"]) == M.GSO_TCPV4
    assert struct.unpack_from(">H", out, o + 2)[0] == int(w["len"]) == 40 + 3 * 1200
    assert M.csum16(out[o:o + 20].tobytes()) == 0xFFFF  # the IPv4 header checksum is valid
    w = writes[1]  # the two segments after the PSH: a chain of their own, no PSH in its header
    assert int(w["nseg"]) == 2 and not out[int(w["out_off"]) + 20 + 13] & M.PSH


def test_single_write_is_data_valid_original_bytes():
    d = K.seg(0) + b"\x99" * 7  # untrimmed
    writes, out, pw, ps = run_host([K.P(d, 1)])
    w = writes[0]
    assert (int(w["vnet_flags"]), int(w["gso_type"]), int(w["hdr_len"]), int(w["gso_size"]), int(w["csum_start"]),
            int(w["csum_offset"])) == (2, 0, 0, 0, 0, 0)
    assert out[:len(d)].tobytes() == d and int(w["len"]) == len(d) and list(pw) == [0] and list(ps) == [0]


# ---- checksum seeds (checksum_seed_test.go) ------------------------------------------------------------
def test_fold_once_no_invert_model():
    assert M.fold_once_no_invert(0) == 0
    assert M.fold_once_no_invert(0xFFFF) == 0xFFFF
    assert M.fold_once_no_invert(0x1FFFE) == 0xFFFF
    assert M.fold_once_no_invert(0x10000) == 1
    assert M.fold_once_no_invert(0xFFFFFFFF) == 0xFFFF
    assert M.pseudo_sum_ipv4(b"\x0a\0\0\1", b"\x0a\0\0\2", 6, 1220) == 0x0A00 + 1 + 0x0A00 + 2 + 6 + 1220
    assert M.pseudo_sum_ipv6(bytes(15) + b"\1", bytes(15) + b"\2", 17, 0x10005) == 1 + 2 + 1 + 5 + 17


@pytest.mark.parametrize("src,dst,v6", [
    (b"\xff\xff\xff\xff", b"\xff\xff\xff\xff", False),  # the sum folds more than once
    (b"\0\0\0\0", b"\0\0\0\0", False),
    (b"\xff" * 16, b"\xff" * 16, True),
    (b"\xff\xfe" + b"\0" * 14, b"\0" * 14 + b"\0\1", True),
    (bytes(16), bytes(16), True),
])
@pytest.mark.parametrize("udp", [False, True])
def test_checksum_seed_edges_through_the_host_form(src, dst, v6, udp):
    """Chains whose pseudo-header sums sit at foldOnceNoInvert's edges (carries, 0xFFFF words)."""
    pk = []
    for i in range(3):
        body = K.pay(1000, i)
        if udp:
            d = (M.udp6 if v6 else M.udp4)(src, dst, 0xFFFF, 0xFFFF, body, **({} if v6 else dict(ident=i)))
        else:
            d = (M.tcp6 if v6 else M.tcp4)(src, dst, 0xFFFF, 0xFFFF, 5 + 1000 * i, body, **({} if v6 else dict(ident=i)))
        pk.append(d)
    model = check(K.seq_(pk))
    w = model[0][0]
    assert w["nseg"] == 3
    ip = 40 if v6 else 20
    l4 = w["len"] - ip
    ps = (M.pseudo_sum_ipv6 if v6 else M.pseudo_sum_ipv4)(src, dst, 17 if udp else 6, l4)
    assert struct.unpack_from(">H", w["data"], ip + (6 if udp else 16))[0] == M.fold_once_no_invert(ps)


# ---- newPacket ----------------------------------------------------------------------------------------
def _ext(nh, n8=1):
    return bytes([nh, n8 - 1]) + bytes(8 * n8 - 2)


def _newpacket_inputs():
    v4 = K.seg(0, n=10)
    out = [b"", b"\x45", v4[:19], v4[:20], v4[:23], v4[:24], b"\x44" + v4[1:], b"\x30" + v4[1:]]
    ic = M.icmp4(K.A, K.B, 1, b"")
    out += [ic[:24], ic[:25], ic[:26], ic]
    out += [M.ipv4(K.A, K.B, 6, b"", frag_off=5), M.ipv4(K.A, K.B, 1, b"ab", mf=True),
            K.seg(0, n=4, options=b"\1" * 8)[:30], K.seg(0, n=4, options=b"\1" * 8)[:32]]
    tcp = M.tcp_hdr(K.A6, K.B6, 1, 2, 3, b"xy")
    for next_ in range(0, 10):  # extension chains of 0-9 headers
        chain, protos = b"", [0, 60, 43, 60, 0, 43, 60, 0, 43][:next_]
        for j in range(next_):
            chain += _ext(protos[j + 1] if j + 1 < next_ else M.TCP, 1 + j % 2)
        out.append(M.ipv6(K.A6, K.B6, protos[0] if next_ else M.TCP, chain + tcp))
    ah = bytes([M.TCP, 4]) + bytes(22)  # AH: (4 + 2) * 4 = 24 bytes
    out += [M.ipv6(K.A6, K.B6, 51, ah + tcp), M.ipv6(K.A6, K.B6, 51, ah[:1]), M.ipv6(K.A6, K.B6, 51, ah + tcp[:3])]
    out += [K.v6_frag_first(M.TCP, tcp), K.v6_frag_first(M.TCP, tcp[:2]),
            M.ipv6(K.A6, K.B6, 44, bytes([M.TCP, 0, 0, 9]) + bytes(4) + b"zz"),   # non-first fragment
            M.ipv6(K.A6, K.B6, 44, bytes([M.TCP, 0, 1, 0]) + bytes(4)),
            M.ipv6(K.A6, K.B6, 44, bytes(7))]
    out += [M.ipv6(K.A6, K.B6, 0, _ext(M.TCP, 4)[:10]),  # a truncated chain: the header points past the packet
            M.ipv6(K.A6, K.B6, 0, _ext(60)[:1]), M.ipv6(K.A6, K.B6, 0, _ext(132, 2)),  # unknown terminal (SCTP)
            M.ipv6(K.A6, K.B6, 135, b""), M.ipv6(K.A6, K.B6, 59, b"")[:39], M.ipv6(K.A6, K.B6, 59, b"")]
    i6 = M.icmp6(K.A6, K.B6, 3, b"")
    out += [i6[:43], i6[:44], i6[:45], i6[:46], M.ipv6(K.A6, K.B6, 58, bytes([1, 0, 0, 0])),
            M.ipv6(K.A6, K.B6, M.UDP, b"abc"), M.ipv6(K.A6, K.B6, M.UDP, b"abcd")]
    return out


def test_new_packet_derivation():
    """Each input alone, derived parse: dropped (INVALID) exactly when the model's newPacket errors,
    routed by the derived protocol otherwise; then once more beside the caller-supplied parse."""
    inputs = _newpacket_inputs()
    verdicts = [M.new_packet(d) for d in inputs]
    assert sum(v is None for v in verdicts) >= 15 and sum(v is not None for v in verdicts) >= 20
    assert M.new_packet(inputs[-1]) == (M.UDP, False, 40) and M.new_packet(inputs[-2]) is None
    packets = K.seq_(inputs)
    model = check(packets, what="derived")
    assert [s == M.ST_INVALID for s in model[2]] == [v is None for v in verdicts]
    # the same packets with the model's parse handed over as the caller's: same writes for the kept ones
    kept = [K.P(d, i + 1, flags=M.PLAIN_PARSED | (M.PLAIN_FRAG_ANY if v[1] else 0), proto=v[0], ip_hdr_len=v[2])
            for i, (d, v) in enumerate(zip(inputs, verdicts)) if v is not None]
    m2 = check(kept, what="caller parse")
    assert [w["data"] for w in m2[0]] == [w["data"] for w in model[0]]


# ---- round trip through the TX segmentation --------------------------------------------------------------
def _chains(writes, datas):
    """(write index, its segmentation by the TX oracle) of every chain."""
    out = []
    for k, (w, data) in enumerate(zip(writes, datas)):
        if int(w["nseg"]) >= 2:
            out.append((k, S.segment_superpacket(data, int(w["vnet_flags"]), int(w["gso_type"]), int(w["hdr_len"]),
                                                 int(w["gso_size"]), int(w["csum_start"]), int(w["csum_offset"]))))
    assert len(out) >= 20
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_round_trip_through_segmentation(seed):
    packets = K.bulk_batch(seed)
    mw, mpw, mst = M.coalesce(packets)
    members = {}
    for i, k in enumerate(mpw):  # input order is counter order here: members come out in chain order
        members.setdefault(k, []).append(i)
    # the model first: every chain segments back into exactly its packets
    for k, segs in _chains(mw, [w["data"] for w in mw]):
        assert segs == [packets[i]["data"] for i in members[k]], k
    writes, out, pw, ps = run_host(packets)
    K.assert_equal_model((mw, mpw, mst), (writes, out, pw, ps), "bulk")
    datas = [out[int(w["out_off"]):int(w["out_off"]) + int(w["len"])].tobytes() for w in writes]
    for k, segs in _chains(writes, datas):
        assert segs == [packets[i]["data"] for i in members[k]], k


# ---- randomised --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_randomised_mix(seed):
    packets = K.random_batch(seed, 3000)
    model = check(packets, what=f"seed {seed}")
    nseg = [w["nseg"] for w in model[0]]
    assert max(nseg) >= 8 and sum(n >= 2 for n in nseg) >= 50 and M.ST_INVALID in model[2] and M.ST_SKIP in model[2]
    check(packets, M.COALESCE_TCP, what=f"seed {seed} tcp only")


# ---- capacity -----------------------------------------------------------------------------------------
def test_capacity_cuts_in_the_middle_of_a_lane():
    packets = next(p for n, p, _ in CASES if n == "multi_restores_transmission_order") + \
        K.seq_([K.seg(i, sport=1500 + i) for i in range(6)], epoch=5)
    full = M.coalesce(packets)
    nw = len(full[0])
    assert nw == 9
    for mw in (0, 1, 4, nw - 1, nw, nw + 3):
        m = check(packets, max_writes=mw, what=f"max_writes {mw}")
        assert len(m[0]) == min(mw, nw)
        assert m[2].count(M.ST_NO_SPACE) == sum(w["nseg"] for w in full[0][mw:])
    ends = [w["out_off"] + M.align16(w["len"]) for w in full[0]]
    for cap in (0, 15, ends[0] - 1, ends[0], ends[3], ends[4] - 16, ends[-1] - 1, ends[-1]):
        m = check(packets, out_cap=cap, what=f"out_cap {cap}")
        assert len(m[0]) == sum(e <= cap for e in ends)


def test_bad_arguments_write_nothing():
    plain, arena = K.stage(K.seq_([K.seg(0), K.seg(1)]))
    out = np.full(8192, 0x77, np.uint8)
    writes = np.zeros(2, L.TUN_WRITE_DTYPE)
    nw = C.c_uint32(99)
    pw = np.full(2, 5, np.uint32)
    ps = np.full(2, 5, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    f = L.lib().neb_rx_coalesce_batch_host
    bad = plain.copy()
    bad[1]["len"] = arena.nbytes  # off + len beyond the arena
    assert f(vp(bad), 2, vp(arena), arena.nbytes, vp(out), out.nbytes, vp(writes), 2, C.byref(nw), vp(pw), vp(ps), 3) \
        == L.ERR_INVALID
    bad = plain.copy()
    bad[0]["off"] = 2**63
    assert f(vp(bad), 2, vp(arena), arena.nbytes, vp(out), out.nbytes, vp(writes), 2, C.byref(nw), vp(pw), vp(ps), 3) \
        == L.ERR_INVALID
    assert f(vp(plain), 2, vp(arena), arena.nbytes, vp(out), out.nbytes, vp(writes), 2, C.byref(nw), vp(pw), vp(ps), 4) \
        == L.ERR_INVALID
    assert f(vp(plain), 2, vp(arena), arena.nbytes, vp(out), out.nbytes, vp(writes), 2, None, vp(pw), vp(ps), 3) \
        == L.ERR_INVALID
    assert (out == 0x77).all() and nw.value == 99 and (pw == 5).all() and (ps == 5).all() and not writes["len"].any()
    assert L.lib().neb_rx_coalesce_batch(None, None, 0, None, None, 0, None, 0, None, None, None, 3, None) == L.ERR_INVALID
    # a skipped record's offset is not looked at
    bad = plain.copy()
    bad[0]["off"], bad[0]["flags"] = 2**63, L.PLAIN_SKIP
    assert f(vp(bad), 2, vp(arena), arena.nbytes, vp(out), out.nbytes, vp(writes), 2, C.byref(nw), vp(pw), vp(ps), 3) == 0
    assert nw.value == 1 and list(ps) == [L.STATUS_NOT_MESSAGE, 0]


def test_empty_batch():
    writes, out, pw, ps = O.coalesce_batch_host(np.zeros(0, L.PLAIN_PACKET_DTYPE), np.zeros(1, np.uint8))
    assert len(writes) == 0 and len(pw) == 0


# ---- the Python mirror ---------------------------------------------------------------------------------
def test_multicoalescer_commit_flush():
    m = O.MultiCoalescer()
    for i in (2, 0, 1):
        m.Commit(K.seg(i), 1, 10 + i)
    m.Commit(K.dgram(0), 1, 5, (M.UDP, False, 20))
    ws = m.Flush()
    assert [(w.lane, w.nseg, w.flags) for w in ws] == [(0, 3, 1), (1, 1, 2)]
    assert ws[0].gso_size == 1200 and ws[0].hdr_len == 40 and ws[0].csum_start == 20 and ws[0].csum_offset == 16
    assert ws[1].data == K.dgram(0) and m.Flush() == []


# ---- wire to plain -------------------------------------------------------------------------------------
def test_plain_from_wire_host():
    from nebula_amd import header as Hd

    rows = [  # (type, subtype, status, key_id, body length)
        (1, 0, 0, 0, 100), (1, 0, 0, 2, 0), (1, 1, 0, 1, 64), (Hd.Test, 0, 0, 1, 64), (Hd.LightHouse, 0, 0, 1, 64),
        (Hd.Control, 0, 0, 0, 40), (Hd.CloseTunnel, 0, 0, 2, 8),
        (1, 0, L.STATUS_AUTH_FAILED, 0, 100), (1, 0, L.STATUS_REPLAY, 1, 100), (1, 0, L.STATUS_BAD_KEY, 0xFFFFFFFF, 50),
        (1, 0, 0, 3, 100), (1, 0, 0, 0xFFFFFFFF, 100), (0, 0, L.STATUS_NOT_MESSAGE, 0, 30), (1, 0, 0, 1, 1300)]
    epoch = [7, 2**40 + 5, 9]
    arena, pk, st = bytearray(b"\x11" * 5), [], []
    for i, (t, sub, status, key, n) in enumerate(rows):
        pk.append((len(arena), 16 + n + 16, key))
        st.append(status)
        arena += Hd.Encode(None, 1, t, sub, 1234 + i, 2**33 + 17 * i) + bytes([i] * n) + bytes(16)
    pkt = np.array(pk, L.RX_PACKET_DTYPE)
    a = np.frombuffer(bytes(arena), np.uint8)
    got = O.plain_from_wire_host(pkt, np.array(st, np.int32), np.array(epoch, np.uint64), a)
    want = M.plain_from_wire(pk, st, epoch, bytes(arena))
    assert sum(not w["flags"] for w in want) == 3
    for g, w in zip(got, want):
        assert (int(g["off"]), int(g["len"]), int(g["counter"]), int(g["epoch"]), int(g["flags"])) == \
            (w["off"], w["len"], w["counter"], w["epoch"], w["flags"])
        assert int(g["proto"]) == 0 and int(g["ip_hdr_len"]) == 0
    bad = pkt.copy()
    bad[3]["len"] = a.nbytes
    plain = np.zeros(len(pk), L.PLAIN_PACKET_DTYPE)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ep = np.array(epoch, np.uint64)
    s32 = np.array(st, np.int32)
    assert L.lib().neb_rx_plain_from_wire_host(vp(bad), vp(s32), vp(ep), 3, len(pk), vp(a), a.nbytes, vp(plain)) \
        == L.ERR_INVALID
    assert not plain["len"].any()
