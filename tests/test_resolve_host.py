"""CPU: neb_index_table_* and neb_rx_resolve_batch_host against the dict model (tests/resolve_ref.py)
on the cases of tests/resolve_cases.py; update semantics, forced rebuilds, and every argument the
calls refuse."""
import ctypes as C
import random

import numpy as np
import pytest

import resolve_cases as RC
import resolve_ref as M
from nebula_amd import _lib as L
from nebula_amd.hostmap import IndexTable, entries


def check(case, model, pk, route, via, n=None, with_src=True):
    keys, lens, routes, vias = RC.expected(model, case, n, with_src)
    assert pk["key_id"].tolist() == keys
    assert pk["len"].tolist() == lens
    assert pk["off"].tolist() == [case.packets[i % len(case.packets)][0] for i in range(len(pk))]
    if route is not None:
        assert [tuple(r) for r in route.tolist()] == routes
    if via is not None:
        assert [tuple(v) for v in via.tolist()] == vias


@pytest.mark.parametrize("capacity", [8, 4096])
def test_host_form_equals_model(capacity):
    case = RC.build(capacity, filler=1000 if capacity > 8 else 0)
    with IndexTable(None, capacity) as t:
        RC.load(t, case)
        arena = case.arena.copy()
        pk, src = RC.packet_array(case)
        route, via = t.resolve_host(pk, arena, src)
        check(case, case.model, pk, route, via)
        assert np.array_equal(arena, case.arena)
        # without sources: the caller's bit stays, none is added
        pk, _ = RC.packet_array(case)
        route, via = t.resolve_host(pk, arena, None, want_route=False)
        assert route is None
        check(case, case.model, pk, None, via, with_src=False)
        route, via = t.resolve_host(pk, arena, None, want_via=False)
        assert via is None
        # a /0 prefix: every 4-byte source, no 16-byte one
        t.set_own_networks(RC.NETS_ZERO)
        zero = case.model.copy()
        zero.set_own_networks(RC.NETS_ZERO)
        pk, src = RC.packet_array(case, 100)
        route, via = t.resolve_host(pk, arena, src)
        check(case, zero, pk, route, via, 100)
        t.set_own_networks([])
        zero.set_own_networks([])
        pk, src = RC.packet_array(case)
        check(case, zero, pk, *t.resolve_host(pk, arena, src))


def test_update_semantics():
    with IndexTable(None, 4) as t:
        rows = [(M.TUNNEL, 10, 1, 0, M.RELAY_NONE, 0), (M.RELAY, 10, 2, 1, 3, 99), (M.TUNNEL, 11, 3, 0, M.RELAY_NONE, 0)]
        t.update([], rows)
        assert t.count() == 3
        # a put of a live key replaces its record; the order inside one call is deletions, then puts
        t.update([(M.TUNNEL, 10)], [(M.TUNNEL, 10, 7, 0, M.RELAY_NONE, 0), (M.TUNNEL, 10, 8, 0, M.RELAY_NONE, 0)])
        assert t.count() == 3 and t.probe(M.TUNNEL, 10)[0]
        # deleting an absent key is not an error
        t.update([(M.TUNNEL, 999), (M.RELAY, 11)], [])
        assert t.count() == 3
        t.update([], [(M.RELAY, 12, 4, 0, M.RELAY_NONE, 0)])
        assert t.count() == 4
        # over capacity: nothing of the call is applied, neither its deletions nor its first puts
        with pytest.raises(L.NebError) as ei:
            t.update([(M.TUNNEL, 11)], [(M.TUNNEL, 20, 1, 0, M.RELAY_NONE, 0), (M.TUNNEL, 21, 1, 0, M.RELAY_NONE, 0)])
        assert ei.value.rc == L.ERR_NO_KEY_SLOT
        assert t.count() == 4 and t.probe(M.TUNNEL, 11)[0] and not t.probe(M.TUNNEL, 20)[0]
        # at capacity: a delete makes room for a put in the same call, a replace needs none
        t.update([(M.TUNNEL, 11)], [(M.TUNNEL, 20, 5, 0, M.RELAY_NONE, 0), (M.RELAY, 10, 6, 0, M.RELAY_NONE, 0)])
        assert t.count() == 4
        hdr = RC.header
        arena = np.frombuffer(hdr(1, 1, 0, 10) + hdr(1, 1, 1, 10) + hdr(1, 1, 0, 11) + hdr(1, 1, 0, 20), np.uint8).copy()
        pk = np.zeros(4, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"] = [0, 16, 32, 48], 16
        route, via = t.resolve_host(pk, arena)
        assert pk["key_id"].tolist() == [8, 6, M.MIXED, 5]
        assert route.tolist() == [(M.RELAY_NONE, 0)] * 4 and via.tolist() == [(M.MIXED, 0)] * 4


def _same_as_model(t, m):
    """One 16-byte packet per live key and a few absent ones, resolved by the table and by the dict."""
    keys = list(m.entries) + [(M.TUNNEL, 1), (M.RELAY, 2), (M.RELAY, 0xFFFFFFFF)]
    arena = np.frombuffer(b"".join(RC.header(1, 1, s, i) for s, i in keys), np.uint8).copy()
    pk = np.zeros(len(keys), L.RX_PACKET_DTYPE)
    pk["off"], pk["len"] = np.arange(len(keys)) * 16, 16
    route, via = t.resolve_host(pk, arena)
    want = m.resolve(arena, [(16 * k, 16) for k in range(len(keys))])
    assert pk["key_id"].tolist() == want[0]
    assert [tuple(r) for r in route.tolist()] == want[2] and [tuple(v) for v in via.tolist()] == want[3]
    assert t.count() == len(m.entries)


def test_three_forced_rebuilds_keep_the_table():
    """Replaces and deletes leave tombstones, which are never reused, so the search for a key that
    every call replaces only ever gets longer; it gets shorter when the table has rebuilt itself
    without them. Through three such rebuilds the table equals the dict after every call."""
    cap = 8
    rng = random.Random(5)
    hot = (M.TUNNEL, 0x01020304)
    with IndexTable(None, cap) as t:
        m = M.Model()
        rebuilds, last, steps = 0, 0, 0
        while rebuilds < 3:
            steps += 1
            assert steps < 200
            live = [k for k in m.entries if k != hot]
            delete, put = [], [(hot[0], hot[1], steps, 0, M.RELAY_NONE, 0)]
            if live and rng.random() < 0.5:
                delete.append(live.pop(rng.randrange(len(live))))
            if len(live) < cap - 1 and rng.random() < 0.7:
                space = rng.randrange(2)
                put.append((space, rng.getrandbits(32), rng.getrandbits(12), rng.randrange(2) * space,
                            rng.choice([M.RELAY_NONE, 3]) if space else M.RELAY_NONE, rng.getrandbits(32)))
            elif live:
                s, i = rng.choice(live)  # replace another record
                put.append((s, i, rng.getrandbits(12), 0, M.RELAY_NONE, 0))
            t.update(delete, put)
            m.update(delete, put)
            found, _, probes = t.probe(*hot)
            assert found
            rebuilds += probes < last
            last = probes
            _same_as_model(t, m)
        assert steps > 3 * 4  # each took a run of calls to fill 3/4 of the slots


def test_invalid_arguments():
    lib = L.lib()
    h = C.c_void_p()
    assert lib.neb_index_table_create(None, 0, C.byref(h)) == L.ERR_INVALID
    assert lib.neb_index_table_create(None, 8, None) == L.ERR_INVALID
    assert lib.neb_index_table_destroy(None) == L.ERR_INVALID
    with IndexTable(None, 8) as t:
        bad = [
            [(2, 1, 1, 0, M.RELAY_NONE, 0)],  # space > 1
            [(M.TUNNEL, 1, 1, M.VIA_TERMINAL, M.RELAY_NONE, 0)],  # a tunnel entry with flags
            [(M.TUNNEL, 1, 1, 0, 3, 0)],  # a tunnel entry with a route
        ]
        for rows in bad:
            with pytest.raises(L.NebError) as ei:
                t.update([], [(M.TUNNEL, 5, 1, 0, M.RELAY_NONE, 0)] + rows)
            assert ei.value.rc == L.ERR_INVALID
        with pytest.raises(L.NebError) as ei:
            t.update([(2, 1)], [(M.TUNNEL, 5, 1, 0, M.RELAY_NONE, 0)])
        assert ei.value.rc == L.ERR_INVALID
        assert t.count() == 0  # nothing of a refused call is applied
        e = entries([(M.TUNNEL, 5, 1, 0, M.RELAY_NONE, 0)])
        assert lib.neb_index_table_update(t.handle, None, 1, None, 0, None) == L.ERR_INVALID
        assert lib.neb_index_table_update(t.handle, None, 0, None, 1, None) == L.ERR_INVALID
        assert lib.neb_index_table_update(None, None, 0, e.ctypes.data_as(C.c_void_p), 1, None) == L.ERR_INVALID
        # own networks: more than 16, a family that is neither, bits beyond the family's width
        nets = np.zeros(17, L.CIDR_DTYPE)
        nets["family"] = 4
        assert lib.neb_index_table_set_own_networks(t.handle, nets.ctypes.data_as(C.c_void_p), 17, None) == L.ERR_INVALID
        assert lib.neb_index_table_set_own_networks(t.handle, nets.ctypes.data_as(C.c_void_p), 16, None) == L.OK
        assert lib.neb_index_table_set_own_networks(t.handle, None, 1, None) == L.ERR_INVALID
        for family, bits in ((4, 33), (6, 129), (0, 0), (5, 8)):
            one = np.zeros(1, L.CIDR_DTYPE)
            one["family"], one["bits"] = family, bits
            assert lib.neb_index_table_set_own_networks(t.handle, one.ctypes.data_as(C.c_void_p), 1, None) == L.ERR_INVALID
        for family, bits in ((4, 32), (6, 128)):
            one = np.zeros(1, L.CIDR_DTYPE)
            one["family"], one["bits"] = family, bits
            assert lib.neb_index_table_set_own_networks(t.handle, one.ctypes.data_as(C.c_void_p), 1, None) == L.OK
        out = (C.c_uint32 * 3)()
        assert lib.neb_index_table_probe(t.handle, 2, 1, out) == L.ERR_INVALID
        assert lib.neb_index_table_probe(None, 0, 1, out) == L.ERR_INVALID
        assert lib.neb_index_table_count(t.handle, None) == L.ERR_INVALID
        # the host form checks every packet against the arena first and then writes nothing
        t.update([], [(M.TUNNEL, 7, 1, 0, M.RELAY_NONE, 0)])
        arena = np.frombuffer(RC.header(1, 1, 0, 7) * 2, np.uint8).copy()
        pk = np.zeros(2, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = [0, 16], [16, 17], 0x55
        route = np.full(2, 0x66, L.RELAY_ROUTE_DTYPE)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert lib.neb_rx_resolve_batch_host(t.handle, vp(pk), None, 2, vp(arena), 32, vp(route), None) == L.ERR_INVALID
        pk["len"] = [16, 16]
        pk["off"] = [0, 33]
        assert lib.neb_rx_resolve_batch_host(t.handle, vp(pk), None, 2, vp(arena), 32, vp(route), None) == L.ERR_INVALID
        assert pk["key_id"].tolist() == [0x55, 0x55] and route["tunnel"].tolist() == [0x66, 0x66]
        assert lib.neb_rx_resolve_batch_host(None, vp(pk), None, 2, vp(arena), 32, None, None) == L.ERR_INVALID
        assert lib.neb_rx_resolve_batch_host(t.handle, None, None, 2, vp(arena), 32, None, None) == L.ERR_INVALID
        assert lib.neb_rx_resolve_batch_host(t.handle, None, None, 0, None, 0, None, None) == L.OK  # n == 0
        pk["off"], pk["len"] = [0, 32], [16, 0 | M.OWN_SOURCE]  # a flagged empty packet at the arena's end
        assert lib.neb_rx_resolve_batch_host(t.handle, vp(pk), None, 2, vp(arena), 32, vp(route), None) == L.OK
        assert pk["key_id"].tolist() == [1, M.MIXED] and pk["len"].tolist() == [16, M.OWN_SOURCE]
        # the device form refuses a host-only table (and a missing engine) before it touches a device
        assert lib.neb_rx_resolve_batch(None, t.handle, vp(pk), None, 2, vp(arena), None, None, None) == L.ERR_INVALID
