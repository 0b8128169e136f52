"""TEST INFRASTRUCTURE ONLY: the seeded case builder of the receive resolve, for
tests/test_resolve_cases.py, tests/test_resolve_host.py and tests/test_gpu_resolve.py.

build(capacity) searches, on a host-only table through neb_index_table_probe, for local indexes
whose slots collide the way the coverage list of tests/test_resolve_cases.py asks, and lays out a
receive batch over them. Nothing here knows the table's hash: a key's home slot is where an empty
table's search for it ends."""
import functools
import random
from types import SimpleNamespace

import numpy as np

import resolve_ref as M
from nebula_amd import _lib as L
from nebula_amd.hostmap import IndexTable, sources

LENGTHS = (0, 1, 15, 16, 31, 32, 47, 48, 49, 1364)
NETS_MAIN = ("0.0.0.0/1", "203.0.113.0/24", "198.51.100.7/32", "2001:db8:8000::/33", "fd00:1:2:3::/64", "fd00::9/128")
NETS_ZERO = ("0.0.0.0/0",)  # every 4-byte address, no 16-byte one
# (source, inside NETS_MAIN); None: family 0
SOURCES = (("10.1.2.77", True), ("200.1.1.1", False), ("203.0.113.9", True), ("198.51.100.7", True),
           ("198.51.100.8", False), ("2001:db8:8000::1", True), ("2001:db8:7fff::1", False), ("fd00:1:2:3::5", True),
           ("fd00:1:2:4::5", False), ("fd00::9", True), ("fd00::a", False), ("::ffff:203.0.113.9", False),
           ("::ffff:10.1.2.77", False), (None, False))


def header(version, typ, sub, index, counter=7):
    return bytes([(version << 4) | typ, sub, 0, 0]) + index.to_bytes(4, "big") + counter.to_bytes(8, "big")


def slots_of(capacity):
    """The table's slot count as include/nebula_aead.h's sizing note gives it."""
    s = 16
    while s < 4 * capacity:
        s *= 2
    return s


def _search(capacity, rng):
    """Indexes by home slot: three that share one, two at the last slot, two more that share one."""
    empty = IndexTable(None, capacity)
    last = slots_of(capacity) - 1
    homes, seen = {}, set()
    last_relay = last_tunnel = None

    pairs, trios = set(), set()  # homes with at least two / three indexes

    def done():
        return trios and len(pairs) >= 2 and last_relay is not None and last_tunnel is not None

    while not done():
        idx = rng.getrandbits(32)
        if idx in seen:
            continue
        seen.add(idx)
        found, home, probes = empty.probe(M.TUNNEL, idx)
        assert not found and probes == 1
        if home == last:
            last_tunnel = idx if last_tunnel is None else last_tunnel
        elif empty.probe(M.RELAY, idx)[1] == last:
            last_relay = idx if last_relay is None else last_relay
        else:
            b = homes.setdefault(home, [])
            b.append(idx)
            if len(b) == 2:
                pairs.add(home)
            elif len(b) == 3:
                trios.add(home)
    empty.close()
    by_size = sorted(homes.values(), key=len, reverse=True)
    return by_size[0][:3], (last_relay, last_tunnel), by_size[1][:2]


@functools.lru_cache(maxsize=None)  # shared between the tests: treat the result as read-only
def build(capacity, seed=20260901, filler=0):
    """Returns a namespace: updates (the update calls, in order: [(delete, put rows)]), model (the
    dict model after them), arena, packets [(off, len)], srcs / src_array, names (what each role's
    index is) and which packet shows what (roles)."""
    rng = random.Random(seed * 1000003 + capacity)
    (a1, a2, a3), (w1, w2), (b1, b2) = _search(capacity, rng)
    unknown = 0x0BADF00D
    R_TERM, R_FWD = (M.RELAY, a2), (M.RELAY, w1)
    rows1 = [
        (M.TUNNEL, a1, M.MIXED, 0, M.RELAY_NONE, 0),  # a HostInfo without a ConnectionState
        (M.TUNNEL, a2, 2, 0, M.RELAY_NONE, 0),
        (M.TUNNEL, a3, 3, 0, M.RELAY_NONE, 0),  # the chain of three
        (M.RELAY, a2, 5, M.VIA_TERMINAL, M.RELAY_NONE, 0),  # the same index in the other space
        (M.RELAY, w1, 6, 0, 4, 0x51525354),  # forwarding, with a route; home: the last slot
        (M.TUNNEL, b1, 1, 0, M.RELAY_NONE, 0),
        (M.TUNNEL, b2, 7, 0, M.RELAY_NONE, 0),
    ]
    updates = [([], rows1)]
    # w2's home is the last slot too (its own space's hash may differ: the test asserts the wrap)
    updates.append(([(M.TUNNEL, b1), (M.TUNNEL, unknown)], [(M.TUNNEL, w2, 0, 0, M.RELAY_NONE, 0)]))
    fill = []
    while len(fill) < filler:  # other tunnels and relays around them
        idx = rng.getrandbits(32)
        if idx in (a1, a2, a3, w1, w2, b1, b2, unknown):
            continue
        if rng.randrange(2):
            fill.append((M.RELAY, idx, rng.randrange(4096), rng.randrange(2), rng.choice([M.RELAY_NONE, 9]), 77))
        else:
            fill.append((M.TUNNEL, idx, rng.randrange(4096), 0, M.RELAY_NONE, 0))
    if fill:
        updates.append(([], fill))
    model = M.Model()
    for d, p in updates:
        model.update(d, p)
    model.set_own_networks(NETS_MAIN)

    pkts, roles = [], {}

    def add(role, data):
        roles.setdefault(role, []).append(len(pkts))
        pkts.append(bytes(data))

    def pad(head, n):
        body = head + bytes(rng.getrandbits(8) for _ in range(max(n - len(head), 0)))
        return body[:n]

    for n in LENGTHS:  # a direct packet and a terminal relay packet of every length
        add(("direct", n), pad(header(1, 1, 0, a3), n))
        add(("terminal", n), pad(header(1, 1, 1, a2) + header(1, 1, 0, b2), n))
    for typ in range(8):
        for sub in range(3):
            add(("type", typ, sub), pad(header(1, typ, sub, a2), 40))
    add("version", pad(header(2, 1, 0, a2), 40))
    add("version_relay", pad(header(3, 1, 1, a2) + header(1, 1, 0, a3), 64))
    add("relay_in_relay", pad(header(1, 1, 1, a2) + header(1, 1, 1, w1), 80))
    add("inner_unknown", pad(header(1, 1, 1, a2) + header(1, 1, 0, unknown), 80))
    add("forwarding", pad(header(1, 1, 1, w1) + header(1, 1, 0, a3), 80))
    add("relay_miss", pad(header(1, 1, 1, a3), 80))
    add("tunnel_miss", pad(header(1, 1, 0, unknown), 80))
    add("deleted", pad(header(1, 1, 0, b1), 80))
    add("mixed_entry", pad(header(1, 1, 0, a1), 80))
    add("behind_tombstone", pad(header(1, 1, 0, b2), 80))
    add("wrapped", pad(header(1, 1, 0, w2), 80))
    add("chain", pad(header(1, 1, 0, a3), 80))

    # lay out: every residue of off % 16, and headers that straddle a 128-byte line
    arena = bytearray()
    packets = []
    for k, p in enumerate(pkts):
        want = k % 16
        while len(arena) % 16 != want:
            arena.append(0xEE)
        if k % 7 == 3 and want:  # the 16-byte header crosses a 128-byte line
            while len(arena) % 128 != 112 + want:
                arena.append(0xEE)
        packets.append([len(arena), len(p)])
        arena += p
    arena += bytes(16)

    srcs = [SOURCES[k % len(SOURCES)][0] for k in range(len(pkts))]
    src_array = sources(srcs)
    for k, s in enumerate(srcs):
        if s is None:  # family 0 with the bytes of an address that is inside
            src_array[k]["addr"][:4] = (10, 1, 2, 77)
    per = len(SOURCES)
    preset = [k for k, s in enumerate(srcs) if (s == "200.1.1.1" and (k // per) % 2 == 0) or (s == "fd00::a" and (k // per) % 2)]
    for k in preset:  # the caller's own refusal on a packet whose source is outside: kept
        packets[k][1] |= M.OWN_SOURCE
    return SimpleNamespace(capacity=capacity, updates=updates, model=model, arena=np.frombuffer(bytes(arena), np.uint8).copy(),
                           packets=[tuple(p) for p in packets], srcs=srcs, src_array=src_array, roles=roles, preset=preset,
                           names=dict(a1=a1, a2=a2, a3=a3, w1=w1, w2=w2, b1=b1, b2=b2, unknown=unknown))


def load(table, case):
    """The case's update calls on an IndexTable, and its networks."""
    for d, p in case.updates:
        table.update(d, p)
    table.set_own_networks(NETS_MAIN)


def packet_array(case, n=None):
    """RX_PACKET_DTYPE records (key_id preset to garbage) and the matching sources, the case's
    packets repeated up to n."""
    m = len(case.packets)
    n = m if n is None else n
    pk = np.zeros(n, L.RX_PACKET_DTYPE)
    src = np.zeros(n, L.RX_SOURCE_DTYPE)
    for i in range(n):
        pk[i]["off"], pk[i]["len"] = case.packets[i % m]
        pk[i]["key_id"] = 0xABAB0000 + i
        src[i] = case.src_array[i % m]
    return pk, src


def expected(model, case, n=None, with_src=True):
    m = len(case.packets)
    n = m if n is None else n
    packets = [case.packets[i % m] for i in range(n)]
    srcs = [case.srcs[i % m] for i in range(n)] if with_src else None
    return model.resolve(case.arena, packets, srcs)
