"""TEST INFRASTRUCTURE ONLY: the case builder of the RX inner resolve, for
tests/test_rx_inner_cases.py, tests/test_rx_inner_host.py and tests/test_gpu_rx_inner.py.

build() lays out a batch of opened wire packets (header, plaintext, tag room) over a peer table and
a routable set that cover the list in tests/test_rx_inner_cases.py. Every item names the status it
is meant to reach; the model (tests/rx_inner_ref.py) has to agree before anything else is compared.
The keys whose slots collide are found on an empty host-only table through neb_peer_table_probe:
nothing here knows the table's hash."""
import functools
import ipaddress
import struct
from types import SimpleNamespace

import numpy as np

import rx_inner_ref as M
from nebula_amd import _lib as L
from nebula_amd.hostmap import PeerTable, build_networks, routable
from tx_resolve_cases import v4, v6  # packet builders only: v4(dst, src=...), v6(dst, src=...)

CAPACITY = 64
MY_NETWORKS = ("10.1.0.7/16", "fd00:1::7/64")
MY_UNSAFE = ("192.168.50.0/24", "2001:db8:50::/48")
ME4, ME6 = "10.1.0.7", "fd00:1::7"
NEPOCH = 13
EPOCHS = [(k << 32) | (7 + k) for k in range(NEPOCH)]
T_SIMPLE, T_TABLE, T_TWO, T_UNSAFE, T_ZERO, T_ONE, T_NEST, T_A, T_B, T_MAPPED, T_CHAIN, T_EMPTY, T_FLOW = range(13)
AUTH_FAILED = 1

# per tunnel: (the peer certificate's networks, its unsafe networks) for build_networks
CERTS = {
    T_SIMPLE: (["10.1.0.9/16"], []),  # the simple case: the model keeps no table for it
    T_TABLE: (["10.1.0.10/16"], []),  # the same shape, the model keeps its one-entry table
    T_TWO: (["10.1.0.20/16", "172.20.0.5/24", "fd00:1::20/64"], []),  # VPN, VPN_PEER, VPN
    T_UNSAFE: (["10.1.0.30/16"], ["11.0.0.0/8", "12.1.1.0/24", "13.1.1.2/31", "14.1.1.1/32", "2001:db8:1::/48",
                                  "2001:db8:2:3::/64", "2001:db8:4::2/127", "2001:db8:5::5/128"]),
    T_ZERO: (["10.1.0.31/16"], ["0.0.0.0/0"]),
    T_ONE: (["10.1.0.32/16"], ["128.0.0.0/1"]),
    # a VPN_PEER address inside an unsafe network inside a wider one; an unsafe /32 equal to the VPN address
    T_NEST: (["10.1.0.40/16", "172.21.9.5/24"], ["172.16.0.0/12", "172.21.9.0/24", "10.1.0.40/32"]),
    T_MAPPED: (["10.1.0.50/16"], ["::ffff:10.1.0.51/128"]),
    T_FLOW: (["10.1.0.60/16"], []),
}
# the same prefix under two tunnels with different types (not a shape buildNetworks makes: the table takes it)
EXTRA = [(T_A, "30.0.0.0/24", L.NET_UNSAFE), (T_B, "30.0.0.0/24", L.NET_VPN_PEER)]


def wire(payload, counter, typ=1, subtype=0, index=0x01020304):
    """An opened packet as it lies in the arena: header, plaintext, the tag's 16 bytes."""
    return struct.pack(">BBHIQ", 0x10 | typ, subtype, 0, index, counter) + bytes(payload) + b"\xEE" * 16


def tcp4(src, dst, seq, payload, sport=40000, dport=443, flags=0x10):
    tcp = struct.pack(">HHIIBBHHH", sport, dport, seq, 1, 5 << 4, flags, 65535, 0, 0) + payload
    return struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + len(tcp), 0, 0x4000, 64, 6, 0, ipaddress.ip_address(src).packed,
                       ipaddress.ip_address(dst).packed) + tcp


def _parse_items():
    """(name, plaintext, tunnel, want): every newPacket error at its boundary, one byte short and exact."""
    s4, s6, t = "10.1.0.9", "fd00:1::20", T_SIMPLE
    p4 = lambda **kw: v4(ME4, src=s4, **kw)  # noqa: E731
    p6 = lambda **kw: v6(ME6, src=s6, **kw)  # noqa: E731
    out = [("empty_payload", b"", t, M.INVALID), ("v4_len1", p4(cut=1), t, M.INVALID), ("v4_len19", p4(cut=19), t, M.INVALID),
           ("v4_len20_no_ports", p4(cut=20), t, M.INVALID), ("v4_ihl16", p4(ihl=16), t, M.INVALID)]
    for ihl in (20, 24, 40, 60):
        out += [(f"v4_ihl{ihl}_p3", p4(ihl=ihl, cut=ihl + 3), t, M.INVALID), (f"v4_ihl{ihl}_p4", p4(ihl=ihl, cut=ihl + 4), t, M.OK),
                (f"v4_ihl{ihl}_icmp_p5", p4(ihl=ihl, proto=M.ICMP, dport=0xBEEF, cut=ihl + 5), t, M.INVALID),
                (f"v4_ihl{ihl}_icmp_p6", p4(ihl=ihl, proto=M.ICMP, dport=0xBEEF, cut=ihl + 6), t, M.OK)]
    out += [("v4_frag_exact_ihl", p4(ff=185, cut=20), t, M.OK), ("v4_frag_ihl24_short", p4(ihl=24, ff=185, cut=23), t, M.INVALID),
            ("v4_frag_ihl24_exact", p4(ihl=24, ff=0x2000 | 7, cut=24), t, M.OK), ("v4_mf_only", p4(ff=0x2000), t, M.OK),
            ("v4_mf_only_p3", p4(ff=0x2000, cut=23), t, M.INVALID), ("v4_tcp", p4(proto=M.TCP, sport=443, dport=50000), t, M.OK),
            ("v4_proto47_ports", p4(proto=47, sport=0x1111, dport=0x2222), t, M.OK),
            ("v0", p4(version=0), t, M.INVALID), ("v5", p4(version=5), t, M.INVALID), ("v7", p4(version=7), t, M.INVALID)]
    t = T_TWO
    out += [("v6_len39", p6(cut=39), t, M.INVALID), ("v6_len40_nonext", p6(proto=59), t, M.OK), ("v6_udp_p3", p6(cut=43), t, M.INVALID),
            ("v6_udp", p6(sport=5353, dport=53), t, M.OK), ("v6_tcp", p6(proto=M.TCP, sport=1, dport=2), t, M.OK)]
    for ext in ("hop", "rt", "dst", "ah"):
        out += [(f"v6_{ext}", p6(chain=(ext,)), t, M.OK), (f"v6_{ext}_short", p6(chain=(ext,), cut=41), t, M.INVALID),
                (f"v6_{ext}_p3", p6(chain=(ext,), cut=40 + (12 if ext == "ah" else 8) + 3), t, M.INVALID)]
    out += [("v6_frag_first", p6(chain=("frag",)), t, M.OK), ("v6_frag_short", p6(chain=("frag",), cut=47), t, M.INVALID),
            ("v6_frag_later", p6(chain=("hop", "frag_later")), t, M.OK),
            ("v6_frag_later_exact", p6(chain=("frag_later",), cut=48), t, M.OK),
            ("v6_chain8", p6(chain=("hop", "dst", "rt", "dst", "ah", "dst", "dst", "rt")), t, M.OK),
            ("v6_chain9", p6(chain=("hop", "dst", "rt", "dst", "ah", "dst", "dst", "dst", "dst")), t, M.OK),  # proto 60 as is
            ("v6_ext_past_end", p6(chain=("dst",), ext_len=200), t, M.INVALID),
            ("v6_echo_p5", p6(proto=M.ICMP6, dport=0xCAFE, cut=45), t, M.INVALID),
            ("v6_echo_p6", p6(proto=M.ICMP6, dport=0xCAFE, cut=46), t, M.OK),
            ("v6_echo_reply", p6(proto=M.ICMP6, dport=0xCAFE, icmp_type=129), t, M.OK),
            ("v6_nonecho_p3", p6(proto=M.ICMP6, icmp_type=135, cut=43), t, M.INVALID),
            ("v6_nonecho_p4", p6(proto=M.ICMP6, icmp_type=135, cut=44), t, M.OK),
            ("v6_ext_icmp", p6(chain=("hop",), proto=M.ICMP6, dport=9), t, M.OK)]
    return out


def _address_items():
    u = lambda src, dst=ME4, **kw: v4(dst, src=src, **kw)  # noqa: E731
    w = lambda src, dst=ME6, **kw: v6(dst, src=src, **kw)  # noqa: E731
    out = [
        ("simple_ok", u("10.1.0.9"), T_SIMPLE, M.OK), ("simple_other", u("10.1.0.10"), T_SIMPLE, M.BAD_REMOTE),
        ("table_ok", u("10.1.0.10"), T_TABLE, M.OK), ("table_other", u("10.1.0.9"), T_TABLE, M.BAD_REMOTE),
        ("two_vpn", u("10.1.0.20"), T_TWO, M.OK), ("two_vpn_peer", u("172.20.0.5"), T_TWO, M.PEER_REJECTED),
        ("two_vpn6", w("fd00:1::20"), T_TWO, M.OK), ("two_peer_neighbour", u("172.20.0.6"), T_TWO, M.BAD_REMOTE),
        ("spoof_other_tunnels_address", u("10.1.0.9"), T_TWO, M.BAD_REMOTE),
        ("empty_tunnel", u("10.1.0.9"), T_EMPTY, M.BAD_REMOTE),
        ("mapped_vs_v4_entry", w("::ffff:10.1.0.50"), T_MAPPED, M.BAD_REMOTE), ("v4_entry", u("10.1.0.50"), T_MAPPED, M.OK),
        ("mapped_vs_v6_entry", w("::ffff:10.1.0.51"), T_MAPPED, M.OK), ("v4_vs_mapped_entry", u("10.1.0.51"), T_MAPPED, M.BAD_REMOTE),
        ("zero_any", u("203.0.113.1"), T_ZERO, M.OK), ("zero_v6_none", w("2001:db8:1::1"), T_ZERO, M.BAD_REMOTE),
        ("one_in", u("128.0.0.1"), T_ONE, M.OK), ("one_out", u("127.255.255.255"), T_ONE, M.BAD_REMOTE),
        ("nest_12", u("172.16.0.1"), T_NEST, M.OK), ("nest_24", u("172.21.9.6"), T_NEST, M.OK),
        ("nest_peer_wins", u("172.21.9.5"), T_NEST, M.PEER_REJECTED), ("nest_unsafe_over_vpn", u("10.1.0.40"), T_NEST, M.OK),
        ("same_prefix_a", u("30.0.0.9"), T_A, M.OK), ("same_prefix_b", u("30.0.0.9"), T_B, M.PEER_REJECTED),
        ("icmp_orientation", u("10.1.0.9", proto=M.ICMP, dport=0x1234), T_SIMPLE, M.OK),
        ("icmp6_orientation", w("fd00:1::20", proto=M.ICMP6, dport=0x4321), T_TWO, M.OK),
        # the local address
        ("local_own", u("10.1.0.9", dst="10.1.0.7"), T_SIMPLE, M.OK), ("local_own6", w("fd00:1::20", dst="fd00:1::7"), T_TWO, M.OK),
        ("local_unsafe", u("10.1.0.9", dst="192.168.50.9"), T_SIMPLE, M.OK),
        ("local_unsafe6", w("fd00:1::20", dst="2001:db8:50:ffff::1"), T_TWO, M.OK),
        ("local_in_vpn_net_not_own", u("10.1.0.9", dst="10.1.0.8"), T_SIMPLE, M.BAD_LOCAL),
        ("local_in_vpn_net_not_own6", w("fd00:1::20", dst="fd00:1::8"), T_TWO, M.BAD_LOCAL),
        ("local_mapped_own", w("fd00:1::20", dst="::ffff:10.1.0.7"), T_TWO, M.BAD_LOCAL),
        ("remote_and_local_bad", u("10.9.9.9", dst="10.1.0.8"), T_SIMPLE, M.BAD_REMOTE),
        ("peer_and_local_bad", u("172.20.0.5", dst="10.1.0.8"), T_TWO, M.PEER_REJECTED),
        ("invalid_and_spoofed", u("10.9.9.9", cut=21), T_SIMPLE, M.INVALID),
    ]
    # unsafe prefixes by length: the first and last address inside, the neighbours outside
    for net in CERTS[T_UNSAFE][1]:
        n = ipaddress.ip_network(net)
        mk = u if n.version == 4 else w
        out += [(f"unsafe_{net}_first", mk(str(n[0])), T_UNSAFE, M.OK), (f"unsafe_{net}_last", mk(str(n[-1])), T_UNSAFE, M.OK),
                (f"unsafe_{net}_below", mk(str(n[0] - 1)), T_UNSAFE, M.BAD_REMOTE),
                (f"unsafe_{net}_above", mk(str(n[-1] + 1)), T_UNSAFE, M.BAD_REMOTE)]
    return out


def _slots():
    s = 16
    while s < 4 * CAPACITY:
        s *= 2
    return s


SLOTS = _slots()


def _search():
    """Addresses of fd00:1::/64 under T_CHAIN by home slot on an empty table: three that share one,
    two at the last slot (the chain wraps), two more that share one (a live one behind a tombstone)."""
    homes = {}
    with PeerTable(None, CAPACITY) as empty:
        for k in range(0x1000, 0x1000 + 12 * SLOTS):
            a = str(ipaddress.ip_address("fd00:1::") + k)
            found, home, probes = empty.probe(T_CHAIN, a + "/128")
            assert not found and probes == 1 and home < SLOTS
            homes.setdefault(home, []).append(a)
    wrap = homes[SLOTS - 1][:2]
    trio_home = min(h for h, g in homes.items() if len(g) >= 3 and h < SLOTS - 8)
    pair_home = min(h for h, g in homes.items() if len(g) >= 2 and h < SLOTS - 8 and abs(h - trio_home) > 8)
    assert len(wrap) == 2
    return homes[trio_home][:3], wrap, homes[pair_home][:2]


@functools.lru_cache(maxsize=None)
def build():
    trio, wrap, pair = _search()
    # table updates in order: (delete, put)
    base = [(t, p, ty) for t, (nets, unsafe) in CERTS.items() for p, ty in build_networks(MY_NETWORKS, nets, unsafe)] + EXTRA
    ops = [((), base), ((), [(T_CHAIN, a + "/128", L.NET_VPN) for a in trio + wrap]), ((), [(T_CHAIN, pair[0] + "/128", L.NET_VPN)]),
           ((), [(T_CHAIN, pair[1] + "/128", L.NET_UNSAFE)]), ([(T_CHAIN, pair[0] + "/128")], ())]
    payloads = _parse_items() + _address_items()
    payloads += [(f"shape_trio{k}", v6(ME6, src=a), T_CHAIN, M.OK) for k, a in enumerate(trio)]
    payloads += [(f"shape_wrap{k}", v6(ME6, src=a), T_CHAIN, M.OK) for k, a in enumerate(wrap)]
    payloads += [("shape_tombstoned", v6(ME6, src=pair[0]), T_CHAIN, M.BAD_REMOTE),
                 ("shape_behind_tombstone", v6(ME6, src=pair[1]), T_CHAIN, M.OK)]
    # one TCP flow the coalescer merges, a spoofed segment and a misdirected one in its middle
    seg = lambda k, src="10.1.0.60", dst=ME4: tcp4(src, dst, 1000 + 100 * k, bytes([k]) * 100)  # noqa: E731
    payloads += [("flow0", seg(0), T_FLOW, M.OK), ("flow1", seg(1), T_FLOW, M.OK), ("flow_spoofed", seg(2, src="10.1.0.61"), T_FLOW, M.BAD_REMOTE),
                 ("flow_misdirected", seg(2, dst="10.1.0.99"), T_FLOW, M.BAD_LOCAL), ("flow2", seg(2), T_FLOW, M.OK)]
    # (name, wire, key_id, open status, len flag, want)
    items = [(name, wire(p, (k + 1) | (k << 40)), t, M.OK, 0, want) for k, (name, p, t, want) in enumerate(payloads)]
    good = v4(ME4, src="10.1.0.9")
    items += [
        ("not_opened", wire(good, 900), T_SIMPLE, AUTH_FAILED, 0, M.NOT_MESSAGE),
        ("hdr_test", wire(good, 901, typ=4), T_SIMPLE, M.OK, 0, M.NOT_MESSAGE),
        ("hdr_lighthouse", wire(good, 902, typ=3), T_SIMPLE, M.OK, 0, M.NOT_MESSAGE),
        ("hdr_relay", wire(good, 903, subtype=1), T_SIMPLE, M.OK, 0, M.NOT_MESSAGE),
        ("key_id_at_nepoch", wire(good, 904), NEPOCH, M.OK, 0, M.NOT_MESSAGE),
        ("key_id_mixed", wire(good, 905), L.KEYS_MIXED, M.OK, 0, M.NOT_MESSAGE),
        ("len31", wire(b"", 906)[:31], T_SIMPLE, M.OK, 0, M.NOT_MESSAGE),
        ("len32", wire(b"", 907), T_SIMPLE, M.OK, 0, M.INVALID),
        ("own_source_refused", wire(good, 908), T_SIMPLE, M.INVALID, L.RX_OWN_SOURCE, M.NOT_MESSAGE),
        ("own_source_bit_only", wire(good, 909), T_SIMPLE, M.OK, L.RX_OWN_SOURCE, M.OK),  # the bit is not part of the length
        ("last", wire(v4(ME4, src="10.1.0.9", sport=1, dport=2), 910), T_SIMPLE, M.OK, 0, M.OK),
    ]
    # layout: every offset mod 4 and a 16-aligned one; 0xA5 between the packets; the last packet
    # ends on the arena's last byte
    arena, packets, at = bytearray(b"\xA5" * 16), [], 16
    for k, it in enumerate(items):
        while at % 4 != k % 4 or (k % 8 == 0 and at % 16):
            at += 1
        arena.extend(b"\xA5" * (at - len(arena)))
        packets.append((at, len(it[1])))
        arena.extend(it[1])
        at += len(it[1]) + 1
    model = M.Model()
    model.set_routable(routable(MY_NETWORKS, MY_UNSAFE))
    for dl, pt in ops:
        model.update(dl, pt)
    model.set_simple(T_SIMPLE, "10.1.0.9")  # the reference's own form of the simple case
    return SimpleNamespace(items=items, names=[it[0] for it in items], arena=np.frombuffer(bytes(arena), np.uint8).copy(),
                           packets=packets, model=model, ops=ops, trio=trio, wrap=wrap, pair=pair)


def load(t, case, stream=None):
    t.set_routable(routable(MY_NETWORKS, MY_UNSAFE))
    for dl, pt in case.ops:
        t.update(dl, pt, stream=stream)


def packet_arrays(case, n):
    """n opened packets: the case's, repeated -> (RX_PACKET_DTYPE, open statuses)."""
    m = len(case.items)
    pk, st = np.zeros(n, L.RX_PACKET_DTYPE), np.zeros(n, np.int32)
    for i in range(n):
        off, ln = case.packets[i % m]
        _, _, key_id, status, flag, _ = case.items[i % m]
        pk[i] = (off, ln | flag, key_id)
        st[i] = status
    return pk, st


def expected(model, case, n):
    """(plain bytes, fw bytes, statuses) of packet_arrays(case, n) under the model."""
    m = len(case.items)
    one = [model.inner(w, key_id, status, EPOCHS, off=case.packets[k][0], raw_len=len(w) | flag)
           for k, (_, w, key_id, status, flag, _) in enumerate(case.items)]
    return (b"".join(one[i % m][0] for i in range(n)), b"".join(one[i % m][1] for i in range(n)), [one[i % m][2] for i in range(n)])
