"""CPU: the case builder of the receive resolve (tests/resolve_cases.py) covers what it claims, on a
host-only table through neb_index_table_probe: the probe chains, and every packet, header, relay
and source shape the resolve tests rely on."""
import ipaddress

import pytest

import resolve_cases as RC
import resolve_ref as M
from nebula_amd.hostmap import IndexTable


@pytest.fixture(scope="module", params=[8, 4096])
def loaded(request):
    case = RC.build(request.param, filler=1000 if request.param > 8 else 0)
    t = IndexTable(None, request.param)
    RC.load(t, case)
    yield case, t
    t.close()


def test_probe_chains(loaded):
    case, t = loaded
    nm, last = case.names, RC.slots_of(case.capacity) - 1
    assert t.count() == len(case.model.entries)
    found, slot, probes = t.probe(M.TUNNEL, nm["a3"])
    assert found and probes >= 3  # a probe chain of at least 3
    found, slot, probes = t.probe(M.TUNNEL, nm["w2"])
    assert found and probes >= 2 and slot < last  # a chain that wraps past the last slot
    found, slot, probes = t.probe(M.TUNNEL, nm["b2"])
    assert found and probes >= 2 and not t.probe(M.TUNNEL, nm["b1"])[0]  # live behind a tombstone
    # the tombstone is still there: the search for the deleted key walks over it to b2 and beyond
    assert t.probe(M.TUNNEL, nm["b1"])[2] >= 3
    e = case.model.entries
    assert e[(M.TUNNEL, nm["a2"])] != e[(M.RELAY, nm["a2"])]  # one index, two spaces, two records
    assert t.probe(M.TUNNEL, nm["a2"])[0] and t.probe(M.RELAY, nm["a2"])[0]
    assert e[(M.TUNNEL, nm["a1"])][0] == M.MIXED
    assert not t.probe(M.TUNNEL, nm["unknown"])[0] and not t.probe(M.RELAY, nm["unknown"])[0]


def test_packet_shapes(loaded):
    case, _ = loaded
    lens = {ln & ~M.OWN_SOURCE for _, ln in case.packets}
    assert set(RC.LENGTHS) <= lens
    assert {off % 16 for off, _ in case.packets} == set(range(16))
    assert any(off // 128 != (off + 15) // 128 for off, ln in case.packets if ln & ~M.OWN_SOURCE >= 16)
    for typ in range(8):
        for sub in range(3):
            (k,) = case.roles[("type", typ, sub)]
            off, _ = case.packets[k]
            assert case.arena[off] == 0x10 | typ and case.arena[off + 1] == sub
    off, _ = case.packets[case.roles["version"][0]]
    assert case.arena[off] >> 4 != 1


def test_relay_shapes(loaded):
    case, _ = loaded
    keys, lens, routes, vias = RC.expected(case.model, case)
    one = lambda role: case.roles[role][0]  # noqa: E731
    e = case.model.entries
    nm = case.names
    k = one("relay_in_relay")
    assert vias[k] == (e[(M.RELAY, nm["w1"])][0], M.VIA_TERMINAL) and keys[k] == e[(M.RELAY, nm["a2"])][0]
    assert vias[one("inner_unknown")] == (M.MIXED, M.VIA_TERMINAL)
    k = one("forwarding")
    assert routes[k] == (4, 0x51525354) and vias[k] == (M.MIXED, 0) and keys[k] == 6
    k = one("relay_miss")
    assert keys[k] == M.MIXED and routes[k] == (M.RELAY_NONE, 0) and (M.TUNNEL, nm["a3"]) in e
    assert keys[one("tunnel_miss")] == M.MIXED and keys[one("deleted")] == M.MIXED
    assert keys[one("mixed_entry")] == M.MIXED and keys[one("behind_tombstone")] == 7
    # a terminal relay packet too short for an inner header keeps the flag and finds no inner tunnel
    assert vias[one(("terminal", 47))] == (M.MIXED, M.VIA_TERMINAL)
    assert vias[one(("terminal", 48))] == (7, M.VIA_TERMINAL)
    assert keys[one(("direct", 15))] == M.MIXED and keys[one(("direct", 16))] == 3
    # the space follows type and subtype alone
    for typ in range(8):
        for sub in range(3):
            want = e[(M.RELAY if (typ, sub) == (1, 1) else M.TUNNEL, nm["a2"])][0]
            assert keys[one(("type", typ, sub))] == want
    assert keys[one("version")] == 2 and keys[one("version_relay")] == 5


def test_source_shapes(loaded):
    case, _ = loaded
    nets = [ipaddress.ip_network(n) for n in RC.NETS_MAIN]
    assert {n.prefixlen for n in nets if n.version == 4} == {1, 24, 32}
    assert {n.prefixlen for n in nets if n.version == 6} == {33, 64, 128}
    assert [ipaddress.ip_network(n).prefixlen for n in RC.NETS_ZERO] == [0]
    for s, inside in RC.SOURCES:
        assert case.model.own_source(s) == inside, s
    kinds = {(ipaddress.ip_address(s).version, inside) for s, inside in RC.SOURCES if s}
    assert kinds == {(4, True), (4, False), (6, True), (6, False)}
    # 4-in-6 whose low 32 bits lie inside a v4 prefix
    assert ipaddress.ip_address("203.0.113.9") in nets[1] and not case.model.own_source("::ffff:203.0.113.9")
    assert None in case.srcs and all(s in case.srcs for s, _ in RC.SOURCES)
    keys, lens, _, _ = RC.expected(case.model, case)
    assert case.preset
    for k in case.preset:  # caller-set bit, source outside: kept
        assert not case.model.own_source(case.srcs[k]) and case.packets[k][1] & M.OWN_SOURCE and lens[k] & M.OWN_SOURCE
    assert any(ln & M.OWN_SOURCE for ln in lens) and any(not ln & M.OWN_SOURCE for ln in lens)
    zero = case.model.copy()
    zero.set_own_networks(RC.NETS_ZERO)
    assert zero.own_source("200.1.1.1") and not zero.own_source("::ffff:203.0.113.9") and not zero.own_source("fd00::9")
