"""CPU: neb_rx_inner_batch_host and the neb_peer_table_* calls on a host-only table against the model
(tests/rx_inner_ref.py) over the cases of tests/rx_inner_cases.py: the commit record, the
neb_fw_packet and the status byte for byte; through updates that force rebuilds; the error paths,
which apply nothing; and the consistency of its records with the coalescer's own parse."""
import ctypes as C
import random

import numpy as np
import pytest

import rx_inner_cases as RC
import rx_inner_ref as M
from nebula_amd import _lib as L
from nebula_amd import outside as O
from nebula_amd.hostmap import PeerTable, peer_keys, peer_nets

EP = np.array(RC.EPOCHS, np.uint64)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(t, case, model, n=None, arena=None):
    n = len(case.items) if n is None else n
    pk, st = RC.packet_arrays(case, n)
    plain, fw, inner = O.inner_host(t, pk, st, EP, case.arena if arena is None else arena)
    want_plain, want_fw, want_st = RC.expected(model, case, n)
    assert inner.tolist() == want_st
    assert fw.tobytes() == want_fw
    assert plain.tobytes() == want_plain
    return plain, fw, inner


@pytest.fixture()
def table():
    with PeerTable(None, RC.CAPACITY) as t:
        yield t


def test_host_form_equals_model(table):
    case = RC.build()
    RC.load(table, case)
    _check(table, case, case.model)
    _check(table, case, case.model, n=300)
    # without fw and without the status; an empty batch
    pk, st = RC.packet_arrays(case, len(case.items))
    plain, fw, _ = O.inner_host(table, pk, st, EP, case.arena, want_fw=False)
    assert fw is None and plain.tobytes() == RC.expected(case.model, case, len(pk))[0]
    out = np.zeros(len(pk), L.PLAIN_PACKET_DTYPE)
    assert L.lib().neb_rx_inner_batch_host(table.handle, _vp(pk), _vp(st), _vp(EP), len(EP), len(pk), _vp(case.arena),
                                           case.arena.nbytes, _vp(out), None, None) == L.OK
    assert out.tobytes() == plain.tobytes()
    assert L.lib().neb_rx_inner_batch_host(table.handle, None, None, None, 0, 0, None, 0, None, None, None) == L.OK


def test_bytes_outside_the_packets_are_never_read(table):
    """arena_len is the exact extent of the batch (the last packet ends on it); the bytes between the
    packets and the tags' 16 bytes change nothing."""
    case = RC.build()
    RC.load(table, case)
    other = np.full(len(case.arena), 0x5A, np.uint8)
    for (off, ln) in case.packets:
        other[off:off + max(ln - 16, 0)] = case.arena[off:off + max(ln - 16, 0)]
    assert not np.array_equal(other, case.arena)
    _check(table, case, case.model, arena=other)
    assert case.packets[-1][0] + case.packets[-1][1] == len(case.arena)
    pk, st = RC.packet_arrays(case, len(case.items))
    plain = np.full(len(pk), 0x77, np.uint8).repeat(32).view(L.PLAIN_PACKET_DTYPE)
    before = plain.tobytes()
    inner = np.full(len(pk), 77, np.int32)
    assert L.lib().neb_rx_inner_batch_host(table.handle, _vp(pk), _vp(st), _vp(EP), len(EP), len(pk), _vp(case.arena),
                                           len(case.arena) - 1, _vp(plain), None, _vp(inner)) == L.ERR_INVALID
    assert plain.tobytes() == before and set(inner.tolist()) == {77}  # nothing written


def test_error_paths_apply_nothing(table):
    case = RC.build()
    RC.load(table, case)
    live = table.count()
    lib = L.lib()

    def update(dl, pt):
        return lib.neb_peer_table_update(table.handle, _vp(dl), len(dl), _vp(pt), len(pt), None)

    none = peer_keys([])
    good = (20, "10.77.0.0/16", L.NET_UNSAFE)
    for bad in ((20, "10.78.0.0/16", 0), (20, "10.78.0.0/16", 4), (L.KEYS_MIXED, "10.78.0.0/16", L.NET_VPN)):
        assert update(none, peer_nets([good, bad])) == L.ERR_INVALID
    for field, v in (("family", 5), ("bits", 33)):
        pt = peer_nets([good, (20, "10.78.0.0/16", L.NET_VPN)])
        pt[1][field] = v
        assert update(none, pt) == L.ERR_INVALID
        dl = peer_keys([(20, "10.78.0.0/16")])
        dl[0][field] = v
        assert update(dl, peer_nets([good])) == L.ERR_INVALID
    pt6 = peer_nets([(20, "fd00::/64", L.NET_VPN)])
    pt6[0]["bits"] = 129
    assert update(none, pt6) == L.ERR_INVALID
    # over the capacity: refused whole, also when the same call deletes a live key
    room = RC.CAPACITY - live
    many = peer_nets([(21, f"10.{k}.0.0/16", L.NET_UNSAFE) for k in range(room + 2)])
    one_live = peer_keys([(RC.T_A, "30.0.0.0/24")])
    assert update(one_live, many) == L.ERR_NO_KEY_SLOT
    assert table.count() == live and table.probe(RC.T_A, "30.0.0.0/24")[0] and not table.probe(20, "10.77.0.0/16")[0]
    assert update(one_live, many[:room + 1]) == L.OK and table.count() == RC.CAPACITY  # exactly full is fine
    undo = peer_keys([(21, f"10.{k}.0.0/16") for k in range(room + 1)])
    assert update(undo, peer_nets([(RC.T_A, "30.0.0.0/24", L.NET_UNSAFE)])) == L.OK and table.count() == live
    _check(table, case, case.model)  # and the table is what it was
    # the routable set
    nets = np.zeros(L.RX_MAX_ROUTABLE + 1, L.CIDR_DTYPE)
    nets["family"], nets["bits"] = 4, 32
    assert lib.neb_peer_table_set_routable(table.handle, _vp(nets), len(nets)) == L.ERR_INVALID
    assert lib.neb_peer_table_set_routable(table.handle, _vp(nets), L.RX_MAX_ROUTABLE) == L.OK
    nets["bits"][3] = 33
    assert lib.neb_peer_table_set_routable(table.handle, _vp(nets), 4) == L.ERR_INVALID
    assert lib.neb_peer_table_create(None, 0, C.byref(C.c_void_p())) == L.ERR_INVALID
    assert lib.neb_rx_inner_batch(None, table.handle, None, None, None, 0, 0, None, None, None, None, None) == L.ERR_INVALID


def test_updates_force_rebuilds_and_the_model_holds(table):
    """Random deletes, puts and replacements under a tunnel of their own: every put takes a slot, so
    the table rebuilds itself several times (a chain only shrinks in a rebuild); the directed cases
    and the churned tunnel resolve as the model says throughout."""
    case = RC.build()
    RC.load(table, case)
    model = case.model
    rng = random.Random(5)
    churn = RC.NEPOCH - 1  # T_FLOW's tunnel: one more entry of its own stays
    pool = [f"10.{200 + k % 4}.{k}.0/24" for k in range(12)] + ["10.200.0.0/14", "fd00:99::/48"]
    hot = (churn, "10.250.0.0/16")
    last, rebuilds = 0, 0
    for step in range(160):
        dl = [(churn, rng.choice(pool)) for _ in range(rng.randrange(3))]
        pt = [(churn, rng.choice(pool), rng.choice((L.NET_VPN, L.NET_VPN_PEER, L.NET_UNSAFE))) for _ in range(rng.randrange(4))]
        pt.append(hot + (L.NET_UNSAFE,))  # replaced every step: its chain grows until a rebuild
        table.update(dl, pt)
        model.update(dl, pt)
        probes = table.probe(*hot)[2]
        rebuilds += probes < last
        last = probes
        assert table.count() == model.count() + 1
        if step % 20 == 0:
            _check(table, case, model)
            for p in pool:
                a = p.split("/")[0]
                a = a[:-1] + "9" if "." in a else a + "9"
                w = RC.wire(RC.v4(RC.ME4, src=a) if "." in a else RC.v6(RC.ME6, src=a), 5)
                pk = np.zeros(1, L.RX_PACKET_DTYPE)
                pk[0] = (0, len(w), churn)
                _, _, st = O.inner_host(table, pk, np.zeros(1, np.int32), EP, np.frombuffer(w, np.uint8).copy())
                assert st[0] == model.inner(w, churn, 0, RC.EPOCHS)[2], (step, p)
    assert rebuilds >= 2
    model.update([(churn, p) for p in pool] + [hot], ())  # the cached case's model goes back as it was


def test_records_agree_with_the_coalescers_own_parse(table):
    """neb_rx_coalesce_batch_host over this call's records (NEB_PLAIN_PARSED: the shared parse) equals
    the same over neb_rx_plain_from_wire_host's records (the coalescer's own co_new_packet) once the
    refused and unparsable packets are marked NEB_PLAIN_SKIP there."""
    case = RC.build()
    RC.load(table, case)
    for n in (len(case.items), 2 * len(case.items) + 3):
        pk, st = RC.packet_arrays(case, n)
        plain, _, inner = O.inner_host(table, pk, st, EP, case.arena)
        old = O.plain_from_wire_host(pk, st, EP, case.arena)
        marked = (inner != M.OK) & (inner != M.NOT_MESSAGE)
        assert marked.any() and (inner == M.OK).sum() > 50
        assert ((old["flags"] & L.PLAIN_SKIP) != 0).tolist() == (inner == M.NOT_MESSAGE).tolist()  # the same commit rule
        old["flags"][marked] |= L.PLAIN_SKIP
        for lanes in (L.COALESCE_TCP | L.COALESCE_UDP, 0):
            a = O.coalesce_batch_host(plain, case.arena, lanes)
            b = O.coalesce_batch_host(old, case.arena, lanes)
            assert a[0].tobytes() == b[0].tobytes()  # writes
            wb = int(sum((int(w["len"]) + 15) & ~15 for w in a[0]))
            assert a[1][:wb].tobytes() == b[1][:wb].tobytes()  # bytes
            assert a[2].tolist() == b[2].tolist()  # pkt_write
            assert a[3][~marked].tolist() == b[3][~marked].tolist()
        w, out, pw, _ = O.coalesce_batch_host(plain, case.arena)
        for name in ("flow_spoofed", "flow_misdirected", "spoof_other_tunnels_address"):
            assert pw[case.names.index(name)] == L.WRITE_NONE
        if n == len(case.items):  # the flow's three good segments became one TSO write
            f0, f2 = case.names.index("flow0"), case.names.index("flow2")
            assert pw[f0] == pw[f2] != L.WRITE_NONE and w[pw[f0]]["nseg"] == 3
