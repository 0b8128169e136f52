"""TEST INFRASTRUCTURE ONLY: the case builder of the TX resolve, for tests/test_tx_resolve_cases.py,
tests/test_tx_resolve_host.py and tests/test_gpu_tx_resolve.py.

build() lays out a batch of TUN reads over a table of hosts, routes and own networks that covers the
list in tests/test_tx_resolve_cases.py. The addresses whose slots collide are found on an empty
host-only table through neb_tx_table_probe: nothing here knows the table's hash, a key's home slot
is where an empty table's search for it ends."""
import functools
import ipaddress
import struct
from types import SimpleNamespace

import numpy as np

import tx_resolve_ref as M
from nebula_amd.hostmap import TxTable
from nebula_amd.inside import TX_PACKET_DTYPE

HOSTS, ROUTES, GATEWAYS = 64, 16, 32
OWN = ("10.1.0.7/24", "192.0.2.9/32", "fd00:1::7/64")
ME4, ME6 = "10.1.0.7", "fd00:1::7"
ECMP3 = ("10.2.3.0/24", [("10.1.0.40", 1), ("10.1.0.41", 1), ("10.1.0.42", 1)])  # .41 is down
ECMP105 = ("172.16.0.0/12", [("10.1.0.50", 10), ("10.1.0.51", 5)])  # .50 is down
ECMP_DOWN = ("172.32.0.0/16", [("10.1.0.70", 1), ("10.1.0.71", 1), ("10.1.0.72", 1)])  # all down
ROUTES_A = [("10.0.0.0/8", [("10.1.0.30", 1)]), ("10.2.0.0/16", [("10.1.0.31", 1)]), ECMP3, ECMP105, ECMP_DOWN,
            ("0.0.0.0/0", [("10.1.0.60", 1)]),  # a default route in one family only; its gateway is down
            ("203.0.113.0/24", [("198.51.100.5", 1)]), ("198.51.100.5/32", [("10.1.0.30", 1)]),
            ("2001:db8::/32", [("fd00:1::30", 1)]), ("2001:db8:0:1::/64", [("fd00:1::31", 1)]),
            ("2001:db8:0:1::5/128", [("10.1.0.31", 1)])]
ROUTES_B = [("10.0.0.0/8", [("10.1.0.31", 1)]), ("10.2.3.0/24", [("10.1.0.42", 5), ("10.1.0.40", 10)]),
            ("::/0", [("fd00:1::30", 1)]), ("172.16.0.0/12", [("10.1.0.51", 3)])]
BASE_HOSTS = [("10.1.0.20", 1), ("10.1.0.21", 2), ("fd00:1::20", 3), ("10.1.0.30", 4), ("10.1.0.31", 5), ("10.1.0.40", 6),
              ("10.1.0.42", 7), ("10.1.0.51", 8), ("198.51.100.5", 9), ("fd00:1::30", 10), ("fd00:1::31", 11)]
NTUNNELS = 32


def v4(dst, src=ME4, proto=M.UDP, sport=1000, dport=2000, ihl=20, ff=0, cut=None, version=4):
    l4 = struct.pack(">BBHHH", 8, 0, 0, dport, 1) if proto == M.ICMP else struct.pack(">HH", sport, dport) + bytes(8)
    h = struct.pack(">BBHHHBBH4s4s", (version << 4) | (ihl >> 2), 0, max(ihl, 20) + len(l4), 0x1234, ff, 64, proto, 0,
                    ipaddress.ip_address(src).packed, ipaddress.ip_address(dst).packed)
    p = h + bytes(max(ihl, 20) - 20) + l4
    return p if cut is None else p[:cut]


EXT = {"hop": 0, "rt": 43, "frag": 44, "frag_later": 44, "ah": 51, "dst": 60}


def v6(dst, src=ME6, chain=(), proto=M.UDP, sport=1000, dport=2000, cut=None, icmp_type=128, ext_len=0):
    if proto == M.ICMP6:
        l4 = struct.pack(">BBHHH", icmp_type, 0, 0, dport, 1)
    elif proto in (M.TCP, M.UDP):
        l4 = struct.pack(">HH", sport, dport) + bytes(8)
    else:
        l4 = b""
    nh = [EXT[c] for c in chain] + [proto]
    body = b""
    for k, c in enumerate(chain):
        if c == "frag":
            body += struct.pack(">BBHI", nh[k + 1], 0, 1, 7)  # offset 0, M set: the first fragment
        elif c == "frag_later":
            body += struct.pack(">BBHI", nh[k + 1], 0, (185 << 3) | 1, 7)
        elif c == "ah":
            body += bytes([nh[k + 1], 1]) + bytes(10)  # (1 + 2) * 4 bytes
        else:
            body += bytes([nh[k + 1], ext_len]) + bytes(6)
    body += l4
    p = struct.pack(">IHBB16s16s", 6 << 28, len(body), nh[0], 64, ipaddress.ip_address(src).packed,
                    ipaddress.ip_address(dst).packed) + body
    return p if cut is None else p[:cut]


def _packets():
    """[(name, bytes)]: the parse cases, the destinations, the routes; ECMP comes from _ecmp()."""
    hit = "10.1.0.20"
    out = [
        ("v4_len0", b""), ("v4_len1", v4(hit, cut=1)), ("v4_len19", v4(hit, cut=19)), ("v4_len20", v4(hit, cut=20)),
        ("v4_ihl_lt20", v4(hit, ihl=16)), ("v4_ihl24_p3", v4(hit, ihl=24, cut=27)), ("v4_ihl24_p4", v4(hit, ihl=24, cut=28)),
        ("v4_icmp_p5", v4(hit, proto=M.ICMP, dport=0xBEEF, cut=25)), ("v4_icmp_p6", v4(hit, proto=M.ICMP, dport=0xBEEF, cut=26)),
        ("v4_frag_exact_ihl", v4(hit, ff=185, cut=20)), ("v4_frag_exact_ihl24", v4(hit, ihl=24, ff=0x2000 | 7, cut=24)),
        ("v4_mf_first", v4(hit, ff=0x2000)), ("v4_tcp", v4(hit, proto=M.TCP, sport=443, dport=50000)),
        ("v4_proto_47", v4(hit, proto=47)), ("v5", v4(hit, version=5)),
        ("v6_len39", v6("fd00:1::20", cut=39)), ("v6_len40", v6("fd00:1::20", proto=59)),
        ("v6_udp_p3", v6("fd00:1::20", cut=43)), ("v6_udp", v6("fd00:1::20", sport=5353, dport=53)),
        ("v6_hop", v6("fd00:1::20", chain=("hop",))), ("v6_rt", v6("fd00:1::20", chain=("rt",))),
        ("v6_dst", v6("fd00:1::20", chain=("dst",))), ("v6_ah", v6("fd00:1::20", chain=("ah",), proto=M.TCP)),
        ("v6_frag_first", v6("fd00:1::20", chain=("frag",))), ("v6_frag_later", v6("fd00:1::20", chain=("hop", "frag_later"))),
        ("v6_frag_short", v6("fd00:1::20", chain=("frag",), cut=47)),
        ("v6_chain8", v6("fd00:1::20", chain=("hop", "dst", "rt", "dst", "ah", "dst", "dst", "dst", "dst"), proto=M.UDP)),
        ("v6_ext_past", v6("fd00:1::20", chain=("dst",), ext_len=200)),
        ("v6_echo_p5", v6("fd00:1::20", proto=M.ICMP6, dport=0xCAFE, cut=45)),
        ("v6_echo_p6", v6("fd00:1::20", proto=M.ICMP6, dport=0xCAFE, cut=46)),
        ("v6_echo_reply", v6("fd00:1::20", proto=M.ICMP6, dport=0xCAFE, icmp_type=129)),
        ("v6_nonecho_p3", v6("fd00:1::20", proto=M.ICMP6, icmp_type=135, cut=43)),
        ("v6_nonecho_p4", v6("fd00:1::20", proto=M.ICMP6, icmp_type=135, cut=44)),
        ("v6_ext_icmp", v6("fd00:1::20", chain=("hop",), proto=M.ICMP6, dport=9)),
        # destinations
        ("dst_in_net_hit", v4("10.1.0.21")), ("dst_in_net_miss_under_route", v4("10.1.0.99")), ("dst_in_net6_miss", v6("fd00:1::99")),
        ("dst_self4", v4(ME4)), ("dst_self6", v6(ME6)), ("dst_bcast24", v4("10.1.0.255")), ("dst_bcast32", v4("192.0.2.9")),
        ("dst_mc4", v4("224.0.0.1")), ("dst_mc6", v6("ff02::1")), ("dst_mc4in6", v6("::ffff:224.0.0.1")),
        ("dst_mapped_of_host", v6("::ffff:10.1.0.20")), ("dst_invalid_self", v4(ME4, cut=21)),
        # routes
        ("route_8", v4("10.9.9.9")), ("route_16", v4("10.2.9.9")), ("route_32_and_host", v4("198.51.100.5")),
        ("route_gw_is_that_host", v4("203.0.113.77")), ("route_default_gw_down", v4("8.8.8.8")),
        ("route6_32", v6("2001:db8:5::1")), ("route6_64", v6("2001:db8:0:1::9")), ("route6_128_gw4", v6("2001:db8:0:1::5")),
        ("route6_none", v6("2001:dead::1")), ("route_frag_ports0", v4("10.2.3.9", ff=185)),
    ]
    return out


def _ecmp():
    """Port pairs on the bucket bounds of the two ECMP routes: the hash equal to each bound, and the
    bound plus one, through the inverse of the mixer."""
    out = []
    for name, (prefix, gws), dst in (("ecmp111", ECMP3, "10.2.3.9"), ("ecmp105", ECMP105, "172.20.1.1")):
        bounds = M.buckets([w for _, w in gws])
        for k, b in enumerate(bounds):
            for d in (0, 1):
                if b + d > 0x7FFFFFFF:
                    continue
                for j, (lp, rp) in enumerate(M.unhash_packet(b + d)):
                    assert M.hash_packet(lp, rp) == b + d
                    out.append((f"{name}_bound{k}_plus{d}_{j}", v4(dst, proto=M.TCP if j else M.UDP, sport=lp, dport=rp)))
    out.append(("ecmp_all_down", v4("172.32.1.1", sport=7, dport=8)))
    return out


def _search():
    """Addresses of fd00:1::/64 by home slot on an empty table: three that share one, two at the
    last slot (the chain wraps), two more that share one (a live one behind a tombstone)."""
    homes = {}
    with TxTable(None, HOSTS, ROUTES, GATEWAYS) as empty:
        for k in range(0x1000, 0x1000 + 12 * SLOTS):
            a = str(ipaddress.ip_address("fd00:1::") + k)
            found, home, probes = empty.probe(a)
            assert not found and probes == 1 and home < SLOTS
            homes.setdefault(home, []).append(a)
    wrap = homes[SLOTS - 1][:2]
    trio_home = min(h for h, g in homes.items() if len(g) >= 3 and h < SLOTS - 8)
    pair_home = min(h for h, g in homes.items() if len(g) >= 2 and h < SLOTS - 8 and abs(h - trio_home) > 8)
    assert len(wrap) == 2
    return homes[trio_home][:3], wrap, homes[pair_home][:2]


def _slots():
    s = 16
    while s < 4 * (HOSTS + ROUTES):
        s *= 2
    return s


SLOTS = _slots()


@functools.lru_cache(maxsize=None)
def build():
    trio, wrap, pair = _search()
    # host updates in order: (delete, put)
    ops = [((), BASE_HOSTS), ((), [(a, 12 + k) for k, a in enumerate(trio)]), ((), [(a, 15 + k) for k, a in enumerate(wrap)]),
           ((), [(pair[0], 17)]), ((), [(pair[1], 18)]), ((pair[0],), ())]
    items = _packets() + _ecmp()
    items += [(f"shape_trio{k}", v6(a)) for k, a in enumerate(trio)] + [(f"shape_wrap{k}", v6(a)) for k, a in enumerate(wrap)]
    items += [("shape_tombstoned", v6(pair[0])), ("shape_behind_tombstone", v6(pair[1]))]
    # layout: every in_off mod 4 and a 16-aligned one; 0xA5 between the packets; the last packet,
    # not an empty one, ends on the arena's last byte
    items.append(("last", v4("10.1.0.20", sport=1, dport=2)))
    arena, packets, at = bytearray(b"\xA5" * 16), [], 16
    for k, (name, p) in enumerate(items):
        while at % 4 != k % 4 or (k % 8 == 0 and at % 16):
            at += 1
        arena.extend(b"\xA5" * (at - len(arena)))
        packets.append((at, len(p)))
        arena.extend(p)
        at += len(p) + 1
    model = M.Model()
    model.set_own(OWN, True, True)
    model.set_routes(ROUTES_A)
    for dl, pt in ops:
        model.update_hosts(dl, pt)
    return SimpleNamespace(items=items, names=[n for n, _ in items], arena=np.frombuffer(bytes(arena), np.uint8).copy(),
                           packets=packets, model=model, ops=ops, trio=trio, wrap=wrap, pair=pair)


def load(t, case, routes=ROUTES_A, flags=(True, True)):
    t.set_own(OWN, *flags)
    t.set_routes(routes)
    for dl, pt in case.ops:
        t.update_hosts(dl, pt)


def packet_array(case, n):
    """n TUN reads: the case's packets, repeated; tunnel preset to a value no result has."""
    m = len(case.packets)
    pk = np.zeros(n, TX_PACKET_DTYPE)
    for i in range(n):
        pk[i]["in_off"], pk[i]["len"] = case.packets[i % m]
    pk["tunnel"] = 0xEEEEEEEE
    return pk


def expected(model, case, n):
    """(tunnels, statuses, fw bytes) of packet_array(case, n) under the model."""
    m = len(case.packets)
    one = [model.resolve(bytes(p)) for _, p in case.items]
    return ([one[i % m][0] for i in range(n)], [one[i % m][1] for i in range(n)], b"".join(one[i % m][2] for i in range(n)))
