"""CPU: the directed cases of the RX inner resolve (tests/rx_inner_cases.py) reach what they are
meant to reach, under the model alone (tests/rx_inner_ref.py) — every newPacket error one byte short
and exact, the orientation, the families, the prefix lengths, nesting, the same prefix under two
tunnels, the spoof, the local address, the inputs that are not committed — and the table's chains
have the shapes the case builder looked for. The reference's own test cases
(tests/golden/rx_inner_enforce.json) hold for the model and for the host form."""
import ipaddress
import json
import os
import struct

import numpy as np
import pytest

import rx_inner_cases as RC
import rx_inner_ref as M
from nebula_amd import _lib as L
from nebula_amd import outside as O
from nebula_amd.hostmap import PeerTable, build_networks, routable
from tx_resolve_cases import v4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS = {None: M.OK, "ErrNoMatchingRule": M.OK, "ErrInvalidRemoteIP": M.BAD_REMOTE, "ErrPeerRejected": M.PEER_REJECTED,
          "ErrInvalidLocalIP": M.BAD_LOCAL}


def _by_name(case):
    _, fw, st = RC.expected(case.model, case, len(case.items))
    rec = np.frombuffer(fw, L.FW_PACKET_DTYPE)
    return {n: (st[k], rec[k]) for k, n in enumerate(case.names)}


def test_every_case_reaches_its_status():
    case = RC.build()
    got = _by_name(case)
    assert len(set(case.names)) == len(case.names)
    for name, _, _, _, _, want in case.items:
        assert got[name][0] == want, name
    reached = {s for s, _ in got.values()}
    assert reached == {M.OK, M.INVALID, M.NOT_MESSAGE, M.BAD_REMOTE, M.PEER_REJECTED, M.BAD_LOCAL}


def test_boundaries_come_in_pairs():
    """Every `_p3` / `_p5` / `_short` case fails and its exact-length sibling passes."""
    case = RC.build()
    got = _by_name(case)
    pairs = [(a, a[:-1] + str(int(a[-1]) + 1)) for a in case.names if a.endswith(("_p3", "_p5"))]
    assert len(pairs) >= 12
    for short, exact in pairs:
        if exact in got:
            assert got[short][0] == M.INVALID and got[exact][0] == M.OK, short
    # a failed parse keeps what newPacket had set before it failed
    assert got["v4_ihl24_p3"][1]["ip_hdr_len"] == 24 and got["v4_ihl24_p3"][1]["family"] == 0
    assert got["v4_mf_only_p3"][1]["flags"] == M.FRAG_ANY
    assert got["v6_echo_p5"][1]["ip_hdr_len"] == 40 and got["v6_chain9"][1]["protocol"] == 60


def test_orientation():
    case = RC.build()
    got = _by_name(case)
    udp = got["v4_ihl20_p4"][1]  # v4(): sport 1000, dport 2000, from the peer to us
    assert (udp["remote_port"], udp["local_port"]) == (1000, 2000)
    assert bytes(udp["remote_addr"][:4]) == ipaddress.ip_address("10.1.0.9").packed
    assert bytes(udp["local_addr"][:4]) == ipaddress.ip_address(RC.ME4).packed
    assert (got["v6_udp"][1]["remote_port"], got["v6_udp"][1]["local_port"]) == (5353, 53)
    assert (got["v4_proto47_ports"][1]["remote_port"], got["v4_proto47_ports"][1]["local_port"]) == (0x1111, 0x2222)
    for name, ident in (("icmp_orientation", 0x1234), ("icmp6_orientation", 0x4321)):  # the identifier stays remote
        assert (got[name][1]["remote_port"], got[name][1]["local_port"]) == (ident, 0)
    assert got["v4_frag_exact_ihl"][1]["flags"] == M.FRAGMENT | M.FRAG_ANY and got["v4_mf_only"][1]["flags"] == M.FRAG_ANY


def test_chains_have_the_shapes_looked_for():
    case = RC.build()
    with PeerTable(None, RC.CAPACITY) as t:
        RC.load(t, case)
        assert t.count() == case.model.count() + 1  # the model holds tunnel T_SIMPLE in the reference's simple form
        probes = [t.probe(RC.T_CHAIN, a + "/128") for a in case.trio]
        assert all(f for f, _, _ in probes) and sorted(p for _, _, p in probes)[-1] >= 3
        (f0, s0, _), (f1, s1, p1) = (t.probe(RC.T_CHAIN, a + "/128") for a in case.wrap)
        assert f0 and f1 and s0 == RC.SLOTS - 1 and s1 < 8 and p1 >= 2  # the chain wraps
        assert not t.probe(RC.T_CHAIN, case.pair[0] + "/128")[0]
        found, _, p = t.probe(RC.T_CHAIN, case.pair[1] + "/128")
        assert found and p >= 2  # live behind a tombstone
        # the tunnel is part of the key: the same prefix under another tunnel is another record
        assert t.probe(RC.T_A, "30.0.0.0/24")[0] and t.probe(RC.T_B, "30.0.0.0/24")[0] and not t.probe(RC.T_EMPTY, "30.0.0.0/24")[0]
        assert t.probe(RC.T_A, "30.0.0.77/24")[0]  # host bits are ignored


def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "rx_inner_enforce.json")))["cases"]


@pytest.mark.parametrize("c", _golden(), ids=lambda c: c["name"])
def test_reference_cases_model_and_host_form(c):
    want = ERRORS[c["error"]]
    fp = M.Packet()
    fp.remote, fp.local = ipaddress.ip_address(c["remote"]), ipaddress.ip_address(c["local"])
    nets = M.build_networks(c["my_networks"], c["peer_networks"], c["peer_unsafe"])
    vpn0 = ipaddress.ip_interface(c["peer_networks"][0]).ip
    rt = [ipaddress.ip_network(s) for s in routable(c["my_networks"], c["my_unsafe"])]
    assert M.drop(fp, nets, vpn0, rt) == want
    with PeerTable(None, 8) as t:
        t.set_routable(routable(c["my_networks"], c["my_unsafe"]))
        t.update(put=[(3, p, ty) for p, ty in build_networks(c["my_networks"], c["peer_networks"], c["peer_unsafe"])])
        w = RC.wire(v4(c["local"], src=c["remote"], sport=90, dport=10), 1)
        pk = np.zeros(1, L.RX_PACKET_DTYPE)
        pk[0] = (0, len(w), 3)
        plain, fw, st = O.inner_host(t, pk, np.zeros(1, np.int32), np.arange(4, dtype=np.uint64), np.frombuffer(w, np.uint8).copy())
        assert st[0] == want
        assert (fw[0]["local_port"], fw[0]["remote_port"]) == (10, 90)
        assert bool(plain[0]["flags"] & L.PLAIN_SKIP) == (want != M.OK)


def test_simple_case_equals_its_one_entry_table():
    """h.networks == nil compares with vpnAddrs[0]; a table holding that address at full length as
    NEB_NET_VPN refuses and admits the same packets."""
    mine, peer = ["10.1.0.7/16", "fd00:1::7/64"], ["10.1.0.9/16"]
    assert M.build_networks(mine, peer) is None
    assert build_networks(mine, peer) == [("10.1.0.9/32", L.NET_VPN)]
    table = {ipaddress.ip_network("10.1.0.9/32"): M.VPN}
    rt = [ipaddress.ip_network(s) for s in routable(mine)]
    for remote in ("10.1.0.9", "10.1.0.8", "10.1.0.10", "0.0.0.0", "::ffff:10.1.0.9", "fd00:1::9"):
        for local in ("10.1.0.7", "10.1.0.8", "fd00:1::7"):
            fp = M.Packet()
            fp.remote, fp.local = ipaddress.ip_address(remote), ipaddress.ip_address(local)
            assert M.drop(fp, None, ipaddress.ip_address("10.1.0.9"), rt) == M.drop(fp, table, None, rt)
    # a peer outside our networks, or with more than one network, gets a table
    assert M.build_networks(mine, ["172.20.0.5/24"]) == {ipaddress.ip_network("172.20.0.5/32"): M.VPN_PEER}
    assert M.build_networks(mine, peer, ["10.1.0.9/32"]) == {ipaddress.ip_network("10.1.0.9/32"): M.UNSAFE}
    assert [ty for _, ty in build_networks(mine, peer, ["10.1.0.9/32"])] == [L.NET_VPN, L.NET_UNSAFE]  # put order: the overwrite


def test_binding_constants():
    text = open(os.path.join(ROOT, "include", "nebula_aead.h")).read()
    for name, v in (("NEB_STATUS_RX_BAD_REMOTE", L.STATUS_RX_BAD_REMOTE), ("NEB_STATUS_RX_PEER_REJECTED", L.STATUS_RX_PEER_REJECTED),
                    ("NEB_STATUS_RX_BAD_LOCAL", L.STATUS_RX_BAD_LOCAL), ("NEB_NET_VPN", L.NET_VPN), ("NEB_NET_VPN_PEER", L.NET_VPN_PEER),
                    ("NEB_NET_UNSAFE", L.NET_UNSAFE), ("NEB_RX_MAX_ROUTABLE", L.RX_MAX_ROUTABLE)):
        assert f"#define {name} {v} " in text or f"#define {name} {v}\n" in text, name
    assert (M.BAD_REMOTE, M.PEER_REJECTED, M.BAD_LOCAL) == (L.STATUS_RX_BAD_REMOTE, L.STATUS_RX_PEER_REJECTED, L.STATUS_RX_BAD_LOCAL)
    assert struct.calcsize("<QQQIHBB") == L.PLAIN_PACKET_DTYPE.itemsize
