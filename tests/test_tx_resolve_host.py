"""CPU: neb_tx_resolve_batch_host and the neb_tx_table_* calls on a host-only table against the model
(tests/tx_resolve_ref.py) over the cases of tests/tx_resolve_cases.py: tunnel, status and the
neb_fw_packet byte for byte; through host updates that force rebuilds and through set_routes
replacements; the error paths, which apply nothing."""
import ctypes as C
import random

import numpy as np
import pytest

import tx_resolve_cases as TC
import tx_resolve_ref as M
from nebula_amd import _lib as L
from nebula_amd.hostmap import TxTable, tx_addrs, tx_hosts, tx_own, tx_routes


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(t, case, model, n=None, arena=None):
    n = len(case.items) if n is None else n
    pk = TC.packet_array(case, n)
    fw, st = t.resolve_host(pk, case.arena if arena is None else arena)
    tunnels, statuses, fwb = TC.expected(model, case, n)
    assert st.tolist() == statuses
    assert pk["tunnel"].tolist() == tunnels
    assert fw.tobytes() == fwb
    assert pk["in_off"].tolist() == [case.packets[i % len(case.packets)][0] for i in range(n)]  # nothing else written
    return pk, fw, st


@pytest.fixture()
def table():
    with TxTable(None, TC.HOSTS, TC.ROUTES, TC.GATEWAYS) as t:
        yield t


def test_host_form_equals_model(table):
    case = TC.build()
    TC.load(table, case)
    _check(table, case, case.model)
    _check(table, case, case.model, n=300)
    # without fw; an empty batch
    pk = TC.packet_array(case, len(case.items))
    fw, st = table.resolve_host(pk, case.arena, want_fw=False)
    assert fw is None and st.tolist() == TC.expected(case.model, case, len(pk))[1]
    assert L.lib().neb_tx_resolve_batch_host(table.handle, None, 0, None, 0, None, None) == L.OK


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)])
def test_gates_follow_their_flags(table, flags):
    case = TC.build()
    TC.load(table, case, flags=flags)
    model = case.model.copy()
    model.set_own(TC.OWN, *flags)
    pk, fw, st = _check(table, case, model)
    i = case.names.index("dst_bcast32")  # without the broadcast gate a /32's broadcast address is the own address
    if not flags[0]:
        assert fw[i]["flags"] == M.GATE_SELF
    if not flags[1]:
        assert st[case.names.index("dst_mc4")] == M.NO_TUNNEL  # on to the default route, whose gateway is down


def test_bytes_outside_the_packets_are_never_read(table):
    """in_len is the exact extent of the batch (the last packet ends on it), and the bytes between
    the packets change nothing."""
    case = TC.build()
    TC.load(table, case)
    other = np.full(len(case.arena), 0x5A, np.uint8)
    for (off, ln) in case.packets:
        other[off:off + ln] = case.arena[off:off + ln]
    assert not np.array_equal(other, case.arena)
    _check(table, case, case.model, arena=other)
    pk = TC.packet_array(case, len(case.items))
    before = pk.copy()
    lib = L.lib()
    st = np.full(len(pk), 77, np.int32)
    assert lib.neb_tx_resolve_batch_host(table.handle, _vp(pk), len(pk), _vp(case.arena), len(case.arena) - 1, None,
                                         _vp(st)) == L.ERR_INVALID  # the last packet is one byte over
    assert (pk == before).all() and (st == 77).all()  # (the records have padding: compare fields)
    assert lib.neb_tx_resolve_batch_host(table.handle, _vp(pk), len(pk), _vp(case.arena), len(case.arena), None,
                                         _vp(st)) == L.OK


def test_equal_through_rebuilds_and_route_replacements(table):
    """Host updates alone, with no route replacement in between, until the table has rebuilt itself
    twice (the hot address's chain only shrinks in a rebuild); then route replacements between
    further updates. The host form equals the model after every step."""
    case = TC.build()
    TC.load(table, case)
    model = case.model.copy()
    rng = random.Random(5)
    churn = [f"10.1.0.{k}" for k in range(100, 130)] + [f"fd00:1::{k:x}" for k in range(0x200, 0x20a)]
    hot = "10.1.0.20"

    def step(k):
        dl = rng.sample(churn, 3)
        pt = [(hot, 1)] + [(a, rng.randrange(TC.NTUNNELS)) for a in rng.sample(churn, 6)]
        if k % 7 == 0:  # a gateway's tunnel goes and comes back: no route update needed
            dl.append("10.1.0.30")
        if k % 7 == 3:
            pt.append(("10.1.0.30", 4))
        table.update_hosts(dl, pt)
        model.update_hosts(dl, pt)
        assert len(model.hosts) <= TC.HOSTS

    rebuilds, last = 0, table.probe(hot)[2]
    for k in range(200):  # 7 or 8 slots of 512 per step; a rebuild comes past 384
        step(k)
        probes = table.probe(hot)[2]
        rebuilds += probes < last  # every step replaces the hot address: its chain grows, but for a rebuild
        last = probes
        _check(table, case, model)
        assert table.count() == (len(model.hosts), len(model.routes))
        if rebuilds == 2:
            break
    assert rebuilds == 2
    for k in range(30):
        step(k)
        if k % 10 == 9:
            rows = TC.ROUTES_B if (k // 10) % 2 == 0 else TC.ROUTES_A
            table.set_routes(rows)
            model.set_routes(rows)
        _check(table, case, model)
        assert table.count() == (len(model.hosts), len(model.routes))
    table.set_routes([])
    model.set_routes([])
    _check(table, case, model)


def test_invalid_and_capacity_paths_apply_nothing(table):
    case = TC.build()
    TC.load(table, case)
    lib = L.lib()

    def routes_rc(rows):
        rt = rows if isinstance(rows, np.ndarray) else tx_routes(rows)
        return lib.neb_tx_table_set_routes(table.handle, _vp(rt), len(rt), None)

    gw = [("10.1.0.30", 1)]
    too_many = tx_routes([("10.0.0.0/8", gw)])
    too_many[0]["ngateways"] = L.ROUTE_MAX_GATEWAYS + 1
    bad_family = tx_routes([("10.0.0.0/8", gw)])
    bad_family[0]["gateways"][0]["family"] = 5
    bad_bits = tx_routes([("10.0.0.0/8", gw)])
    bad_bits[0]["bits"] = 33
    bad_prefix_family = tx_routes([("10.0.0.0/8", gw)])
    bad_prefix_family[0]["family"] = 0
    for rows in (too_many, bad_family, bad_bits, bad_prefix_family, [("10.0.0.0/8", [])],
                 [("10.0.0.0/8", [("10.1.0.30", 0), ("10.1.0.31", 0)])],  # total weight 0
                 [("10.0.0.0/8", gw), ("10.3.0.0/8", gw)]):  # the same prefix once masked
        assert routes_rc(rows) == L.ERR_INVALID
    assert routes_rc([(f"10.{k}.0.0/16", gw) for k in range(TC.ROUTES + 1)]) == L.ERR_NO_KEY_SLOT
    assert routes_rc([(f"10.{k}.0.0/16", [(f"10.1.0.{j}", 1) for j in range(16)]) for k in range(3)]) == L.ERR_NO_KEY_SLOT
    assert routes_rc([("10.0.0.0/8", [("10.1.0.30", 0)])]) == L.OK  # a single gateway's weight is not used
    table.set_routes(TC.ROUTES_A)

    bad = tx_hosts([("10.1.0.77", 1), ("10.1.0.78", 2)])
    bad[1]["family"] = 0
    assert lib.neb_tx_table_update_hosts(table.handle, None, 0, _vp(bad), 2, None) == L.ERR_INVALID
    badd = tx_addrs(["10.1.0.20"])
    badd[0]["family"] = 7
    assert lib.neb_tx_table_update_hosts(table.handle, _vp(badd), 1, None, 0, None) == L.ERR_INVALID
    room = TC.HOSTS - table.count()[0]
    over = tx_hosts([(f"10.7.0.{k}", k) for k in range(room + 1)])
    assert lib.neb_tx_table_update_hosts(table.handle, None, 0, _vp(over), len(over), None) == L.ERR_NO_KEY_SLOT
    # deleting as many as the call adds fits; a put of a live address counts once
    fits = tx_hosts([(f"10.7.0.{k}", k) for k in range(room)] + [("10.1.0.20", 1), ("10.1.0.20", 1)])
    assert lib.neb_tx_table_update_hosts(table.handle, None, 0, _vp(fits), len(fits), None) == L.OK
    table.update_hosts([f"10.7.0.{k}" for k in range(room)])

    own = tx_own(TC.OWN)
    assert lib.neb_tx_table_set_own(table.handle, _vp(own), len(own), 4) == L.ERR_INVALID
    bad_own = own.copy()
    bad_own[0]["bits"] = 33
    assert lib.neb_tx_table_set_own(table.handle, _vp(bad_own), len(bad_own), 3) == L.ERR_INVALID
    many = tx_own(["10.1.0.7/24"] * (L.INDEX_MAX_NETWORKS + 1))
    assert lib.neb_tx_table_set_own(table.handle, _vp(many), len(many), 3) == L.ERR_INVALID
    out = C.c_void_p()
    assert lib.neb_tx_table_create(None, 0, 1, 1, C.byref(out)) == L.ERR_INVALID
    _check(table, case, case.model)  # nothing of the above changed a result
    assert table.count() == (len(case.model.hosts), len(TC.ROUTES_A))


def test_device_call_refuses_a_host_only_table(table):
    assert L.lib().neb_tx_resolve_batch(None, table.handle, None, 0, None, None, None, None) in (L.ERR_INVALID,
                                                                                               L.ERR_NO_DEVICE)
