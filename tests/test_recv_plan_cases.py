"""CPU: the RX receive plan's directed cases (tests/recv_plan_cases.py). Every case reaches its stated
condition, the model (tests/recv_plan_ref.py) keeps the plan's own invariants, and the model and the
host form (neb_rx_recv_plan_host) agree with the reference tests' own tables
(tests/golden/recv_plan_deliver.json)."""
import struct

import pytest

import recv_plan_cases as RC
import recv_plan_ref as M
from nebula_amd import _lib as L

DIRECTED = RC.directed()


def _invariants(b, p):
    n = len(b.entries)
    assert len(p.entry_first) == len(p.frm) == n and all(c >= 1 for c in p.count)
    assert p.npackets == len(p.pk) == sum(p.count[:p.done]) <= p.max_packets
    assert all(f != M.NONE for f in p.entry_first[:p.done]) and all(f == M.NONE for f in p.entry_first[p.done:])
    assert p.done == n or p.npackets + p.count[p.done] > p.max_packets
    at = 0
    for j in range(p.done):  # the packets of an entry tile its buffer in order
        assert p.entry_first[j] == at
        e, end = b.entries[j], b.entries[j].off
        for i in range(at, at + p.count[j]):
            assert p.pkt_entry[i] == j and p.pk[i][0] == end and p.src[i] == p.frm[j][:2]
            end += p.pk[i][1]
        assert end == e.off + e.len
        at += p.count[j]


@pytest.mark.parametrize("case", DIRECTED, ids=[c.name for c in DIRECTED])
def test_directed_case(case):
    with_ctrl, with_seg = M.listen_out(case.batch, True), M.listen_out(case.batch, False)
    _invariants(case.batch, with_ctrl)
    _invariants(case.batch, with_seg)
    assert case.reaches(with_ctrl, with_seg), (with_ctrl.seg[:8], with_ctrl.count[:8], with_ctrl.entry_first[:8],
                                               with_ctrl.npackets, with_ctrl.done)
    if case.same:
        assert (with_ctrl.pk, with_ctrl.entry_first, with_ctrl.done) == (with_seg.pk, with_seg.entry_first, with_seg.done)


def test_the_list_covers_every_named_edge():
    names = {c.name for c in DIRECTED}
    for want in ("seg_len_minus_1", "len_0_seg_%d" % RC.INT32_MIN, "width_big_entry_first_is_cut", "entries_70000",
                 "entry_of_65535_middle", "max_packets_entry_boundary", "padding_over_several_workgroups",
                 "v6_socket_unmap_and_neighbours", "ctrl_gro_after_tos", "ctrl_cmsg_len_2_63"):
        assert want in names
    assert len(names) == len(DIRECTED)


def test_random_batches_reach_their_branches():
    cut = split = pad = hostile = 0
    for b in RC.random_batches(20261021, 400):
        c, s = M.listen_out(b, True), M.listen_out(b, False)
        _invariants(b, c)
        _invariants(b, s)
        cut += c.done < len(b.entries)
        split += any(x > 1 for x in c.count)
        pad += c.max_packets > c.npackets
        hostile += c.seg != s.seg
    assert min(cut, split, pad, hostile) > 40


G = RC.golden()


@pytest.mark.parametrize("row", G["deliver_segments"], ids=[r["name"] for r in G["deliver_segments"]])
def test_reference_deliver_segments_table(row):
    n, seg, want = row["payload_len"], row["seg_size"], row["want_lens"]
    got = list(M.deliver_segments(1000, n, seg))
    assert [x[1] for x in got] == want and M.segment_count(n, seg) == len(want)
    assert [x[0] for x in got] == [1000 + sum(want[:k]) for k in range(len(want))]  # tiles the payload, in order
    # the host form, through both inputs of the size, from the reference test's source address
    b = RC.batch([RC.entry(n, seg, off=1000, name=RC.sockaddr4("192.0.2.1", 4242))], lay_out=False)
    for use_ctrl in (True, False):
        p = M.listen_out(b, use_ctrl)
        assert [x[1] for x in p.pk] == want and p.frm[0][2] == 4242
        rc, out, counts = RC.host_plan(b, use_ctrl, len(want))
        assert rc == L.OK
        RC.compare(out, counts, RC.plan_arrays(p, 1), 0)


@pytest.mark.parametrize("row", G["parse_recv_cmsg"], ids=[r["name"] for r in G["parse_recv_cmsg"]])
def test_reference_corrupt_trailers(row):
    ctrl = bytes.fromhex(row["ctrl_hex"])
    assert len(ctrl) == 48 and struct.unpack_from("<qii", ctrl, 0) == (20, M.SOL_UDP, M.UDP_GRO)
    assert M.parse_recv_cmsg(ctrl) == row["want"]
    # the host form: the walk gives 0, so the entry is delivered whole although seg_size says otherwise
    b = RC.batch([RC.entry(3000, 1000, ctrl=ctrl)])
    rc, out, counts = RC.host_plan(b, True, 8)
    assert rc == L.OK and counts.tolist() == [1, 1]
    assert out["pk"].view(L.RX_PACKET_DTYPE)[0].tolist() == (0, 3000, L.KEYS_MIXED)
