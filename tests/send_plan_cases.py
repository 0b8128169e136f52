"""Directed cases of the TX send plan at the edges of the device form's decomposition, shared by the
CPU tests (tests/test_send_plan_cases.py), the host ABI test and the GPU test. Every case states a
condition (`reaches`) over the sequential model's plan and the parallel model's detail, so that a case
which no longer reaches its edge fails instead of passing vacuously.
"""
from __future__ import annotations

import ipaddress
import json
import os
import random
from dataclasses import dataclass
from typing import Callable

import numpy as np

import send_plan_ref as M
from nebula_amd import _lib as L
from nebula_amd import inside as I

OK, NS = M.OK, 1  # a wire_status that is not OK: NEB_STATUS_AUTH_FAILED's value, any would do


def v4(s: str, port: int = 4242):
    return (4, ipaddress.IPv4Address(s).packed + b"\0" * 12, port, 0)


def v6(s: str, port: int = 4242):
    return (6, ipaddress.IPv6Address(s).packed, port, 0)


# The tunnels of the directed cases.
A, B, A_PORT, BAD6, MAPPED, NOADDR, A_AS_6, RELAY, TARGET, A_TWIN, C3 = range(11)
REMOTE = [
    v4("10.0.0.1"),                                              # A
    v4("10.0.0.2"),                                              # B
    v4("10.0.0.1", 4243),                                        # A's address, another port
    v6("2001:db8::1", 9999),                                     # a v6 remote: unroutable on a v4 socket
    v6("::ffff:10.0.0.9"),                                       # 4-in-6: routable on both
    (0, b"\0" * 16, 0, 0),                                       # no valid remote
    (6, ipaddress.IPv4Address("10.0.0.1").packed + b"\0" * 12, 4242, 0),  # A's leading bytes, family 6
    v4("10.0.0.7"),                                              # a relay
    (0, b"\0" * 16, 0, 0),                                       # a target reached through the relay only
    v4("10.0.0.1"),                                              # another tunnel with A's remote
    v4("10.0.0.3"),                                              # C
]
VIA = [M.NONE] * len(REMOTE)
VIA[TARGET] = RELAY


def batch(wires, **kw) -> M.Batch:
    """wires: (len, tunnel[, status[, flags]]); one packet per wire."""
    lens, tun, st, fl = [], [], [], []
    for w in wires:
        lens.append(w[0])
        tun.append(w[1])
        st.append(w[2] if len(w) > 2 else OK)
        fl.append(w[3] if len(w) > 3 else 0)
    kw.setdefault("remote", REMOTE)
    kw.setdefault("via", VIA)
    return M.Batch(lens=lens, packet=list(range(len(lens))), flags=fl, status=st, pkt_tunnel=tun, **kw)


@dataclass
class Case:
    name: str
    batch: M.Batch
    reaches: Callable  # (plan, detail) -> bool


def shape(plan):
    """[(niov, seg_size)] of the entries."""
    return [(e[1], e[2]) for e in plan.entries]


def _plateau_cases():
    out = []
    # k by segments: 63 and 127 (lengths whose byte cap is larger); chunking off
    for ms, ln in ((63, 1000), (127, 500)):
        for n in (ms - 1, ms, ms + 1, 2 * ms):
            want = [(ms, ln)] * (n // ms) + ([(n % ms, ln if n % ms >= 2 else 0)] if n % ms else [])
            out.append(Case(f"plateau_{n}_of_k{ms}", batch([(ln, A)] * n, max_segments=ms, chunk_packets=0),
                            lambda p, d, want=want: shape(p) == want))
    # k by bytes
    for n in (49, 50, 51, 100):
        want = [(50, 1300)] * (n // 50) + ([(n % 50, 1300 if n % 50 >= 2 else 0)] if n % 50 else [])
        out.append(Case(f"plateau_{n}_of_1300B", batch([(1300, A)] * n, chunk_packets=0), lambda p, d, want=want: shape(p) == want))
    out.append(Case("bytes_21667_2_then_1", batch([(21667, A)] * 3), lambda p, d: shape(p) == [(2, 21667), (1, 0)]))
    out.append(Case("bytes_32500_pair", batch([(32500, A)] * 2), lambda p, d: shape(p) == [(2, 32500)]))
    out.append(Case("bytes_32501_alone", batch([(32501, A)] * 2), lambda p, d: shape(p) == [(1, 0)] * 2))
    out.append(Case("bytes_65000_one_each", batch([(65000, A)] * 3), lambda p, d: shape(p) == [(1, 0)] * 3))
    out.append(Case("bytes_65001_one_each", batch([(65001, A)] * 3), lambda p, d: shape(p) == [(1, 0)] * 3))
    return out


def directed() -> list[Case]:
    c = [
        Case("n0", batch([]), lambda p, d: p.entries == [] and p.iov == []),
        Case("n1", batch([(1200, A)]), lambda p, d: p.entries == [(0, 1, 0, A, 1200)] and d["hard"] == [0]),
        Case("n2", batch([(1200, A)] * 2), lambda p, d: p.entries == [(0, 2, 1200, A, 2400)]),
        # every boundary clause alone
        Case("hard_other_destination", batch([(1200, A), (1200, B)]), lambda p, d: d["hard"] == [0, 1]),
        Case("hard_empty_packet", batch([(1200, A), (0, A)]), lambda p, d: d["hard"] == [0, 1] and shape(p) == [(1, 0)] * 2),
        Case("hard_after_empty_packet", batch([(0, A), (0, A)]), lambda p, d: d["hard"] == [0, 1]),
        Case("hard_after_oversize", batch([(65001, A), (65001, A)]), lambda p, d: d["hard"] == [0, 1]),
        Case("hard_after_oversize_shorter", batch([(65001, A), (1200, A), (1200, A)]),
             lambda p, d: d["hard"] == [0, 1] and shape(p) == [(1, 0), (2, 1200)]),
        Case("hard_longer", batch([(600, A), (1200, A)]), lambda p, d: d["hard"] == [0, 1]),
        Case("hard_chunk", batch([(1200, A)] * 3, chunk_packets=2), lambda p, d: d["hard"] == [0, 2] and shape(p) == [(2, 1200), (1, 0)]),
        Case("soft_shorter_joins_and_ends", batch([(1200, A)] * 3 + [(600, A), (600, A)]),
             lambda p, d: d["hard"] == [0] and shape(p) == [(4, 1200), (1, 0)]),
        # absorption and its two refusals
        Case("absorb_below_segment_cap", batch([(1000, A)] * 3 + [(500, A)], max_segments=4), lambda p, d: shape(p) == [(4, 1000)]),
        Case("absorb_refused_by_segment_cap", batch([(1000, A)] * 4 + [(500, A)], max_segments=4),
             lambda p, d: shape(p) == [(4, 1000), (1, 0)] and d["hard"] == [0]),
        Case("absorb_past_the_byte_quotient", batch([(30000, A)] * 2 + [(5000, A)]), lambda p, d: shape(p) == [(3, 30000)]),
        Case("absorb_refused_by_byte_cap", batch([(30000, A)] * 2 + [(5001, A)]),
             lambda p, d: shape(p) == [(2, 30000), (1, 0)] and d["hard"] == [0]),
        Case("plateau_emptied_by_absorption", batch([(1000, A)] * 2 + [(500, A), (400, A), (400, A)]),
             lambda p, d: shape(p) == [(3, 1000), (2, 400)] and any(len(w) == 1 and d["o"][j] == 1 for j, (w, _) in enumerate(d["plateaus"]))),
        Case("gso_off_segments_1", batch([(1200, A)] * 4, max_segments=1), lambda p, d: shape(p) == [(1, 0)] * 4),
        Case("gso_off_segments_0", batch([(1200, A)] * 4, max_segments=0), lambda p, d: shape(p) == [(1, 0)] * 4),
        # NOT_SENT wires
        Case("not_sent_inside_a_run", batch([(1200, A), (1200, A, NS), (1200, A)]), lambda p, d: shape(p) == [(2, 1200)] and p.wire_entry == [0, M.NONE, 0]),
        Case("not_sent_at_the_head", batch([(1200, A, NS), (1200, A), (1200, A)]), lambda p, d: shape(p) == [(2, 1200)] and p.entries[0][0] == 0),
        Case("not_sent_between_plateaus", batch([(1200, A)] * 2 + [(9999, B, NS), (600, A)]), lambda p, d: shape(p) == [(3, 1200)]),
        Case("not_sent_all", batch([(1200, A, NS)] * 3), lambda p, d: p.entries == [] and p.send_status == [M.NOT_SENT] * 3),
        Case("not_sent_with_bad_indexes", M.Batch(lens=[100], packet=[7], flags=[0], status=[NS], pkt_tunnel=[0], remote=REMOTE, via=VIA),
             lambda p, d: p.send_status == [M.NOT_SENT]),
        # routability and destination identity
        Case("mapped_on_v4_socket", batch([(1200, MAPPED)] * 2 + [(1200, BAD6)]), lambda p, d: p.send_status == [OK, OK, M.UNROUTABLE] and shape(p) == [(2, 1200)]),
        Case("v6_socket_takes_all", batch([(1200, MAPPED), (1200, BAD6), (1200, A), (1200, NOADDR)], socket_v4=False),
             lambda p, d: p.send_status == [OK, OK, OK, M.UNROUTABLE]),
        Case("unroutable_breaks_a_run", batch([(1200, A), (1200, BAD6), (1200, A)]), lambda p, d: shape(p) == [(1, 0)] * 2 and p.entries[1][0] == 1),
        Case("family_4_and_6_equal_leading_bytes", batch([(1200, A), (1200, A_AS_6)], socket_v4=False), lambda p, d: shape(p) == [(1, 0)] * 2),
        Case("port_only_differs", batch([(1200, A), (1200, A_PORT)]), lambda p, d: shape(p) == [(1, 0)] * 2),
        Case("two_tunnels_one_remote", batch([(1200, A_TWIN), (1200, A)]), lambda p, d: p.entries == [(0, 2, 1200, A_TWIN, 2400)]),
        Case("via_and_direct_share_a_run", batch([(1264, TARGET, OK, M.WIRE_VIA), (1264, RELAY), (1264, TARGET, OK, M.WIRE_VIA)]),
             lambda p, d: p.entries == [(0, 3, 1264, RELAY, 3 * 1264)]),
        Case("target_without_via_flag_is_unroutable", batch([(1200, TARGET)]), lambda p, d: p.send_status == [M.UNROUTABLE]),
        # out-of-range indexes: packet, tunnel, via
        Case("bad_packet_index", M.Batch(lens=[1200] * 3, packet=[0, 9, 0], flags=[0] * 3, status=[OK] * 3, pkt_tunnel=[A], remote=REMOTE, via=VIA),
             lambda p, d: p.send_status == [OK, M.BAD_KEY, OK] and shape(p) == [(1, 0)] * 2),
        Case("bad_tunnel_index", batch([(1200, A), (1200, len(REMOTE)), (1200, M.NONE), (1200, A)]),
             lambda p, d: p.send_status == [OK, M.BAD_KEY, M.BAD_KEY, OK] and shape(p) == [(1, 0)] * 2),
        Case("bad_via_index", batch([(1200, A, OK, M.WIRE_VIA), (1200, A)]), lambda p, d: p.send_status == [M.BAD_KEY, OK]),
        Case("via_flag_without_via", batch([(1200, TARGET, OK, M.WIRE_VIA), (1200, A)], via=None), lambda p, d: p.send_status == [M.BAD_KEY, OK]),
    ]
    # chunk edges inside a plateau, unroutable wires first so that rank != index
    for ch in (1, 2, 128, 0):
        n = 300 if ch in (128, 0) else 7
        b = batch([(1000, BAD6)] * 3 + [(1000, A)] * n, chunk_packets=ch)

        def reaches(p, d, ch=ch, n=n):
            edges = [i for i in d["hard"] if i > 3]
            if ch == 0:
                return edges == [] and shape(p) == [(63, 1000)] * 4 + [(48, 1000)]
            return edges == [3 + r for r in range(ch, n, ch)] and all(d["rank"][i] != i and d["rank"][i] % ch == 0 for i in edges)
        c.append(Case(f"chunk_{ch}_inside_a_plateau", b, reaches))
    c += _plateau_cases()
    c.append(Case("one_plateau_4097", batch([(100, A)] * 4097, chunk_packets=0), lambda p, d: shape(p) == [(63, 100)] * 65 + [(2, 100)]))
    return c


def parity_chain(drop_first: bool) -> M.Batch:
    """4097 wires to one destination, lengths strictly falling: every run is two packets."""
    w = [(4200 - i, A) for i in range(4097)]
    if drop_first:
        w[0] = (w[0][0], A, NS)
    return batch(w, chunk_packets=0)


def random_batch(rng: random.Random, nmax: int = 40) -> M.Batch:
    n = rng.randrange(0, nmax + 1)
    ndst = rng.randrange(1, 4)
    pool = rng.sample([A, B, A_PORT, BAD6, MAPPED, NOADDR, RELAY, TARGET, A_TWIN, C3], ndst)
    sizes = rng.choice([[0, 1, 65000, 65001, 1200], [1200, 1200, 1200, 600], [32500, 21667, 13000, 1300], [100, 99, 98, 97, 96, 1]])
    wires, ln, dst = [], rng.choice(sizes), rng.choice(pool)
    for _ in range(n):
        r = rng.random()
        if r < 0.25:
            ln = rng.choice(sizes)
        elif r < 0.4:
            ln = max(ln - rng.randrange(0, 3), 0)  # shrinking
        if rng.random() < 0.15:
            dst = rng.choice(pool)
        st = NS if rng.random() < 0.1 else OK
        fl = M.WIRE_VIA if dst == TARGET or rng.random() < 0.03 else 0
        t = dst if rng.random() > 0.02 else len(REMOTE) + 5
        wires.append((ln, t, st, fl))
    return batch(wires, socket_v4=rng.random() < 0.7, max_segments=rng.choice([0, 1, 2, 3, 4, 7, 63]),
                 chunk_packets=rng.choice([0, 1, 2, 3, 5, 8, 128]))


def random_batches(seed: int, count: int, nmax: int = 40):
    rng = random.Random(seed)
    return [random_batch(rng, nmax) for _ in range(count)]


def golden():
    """The reference tests' own shapes (tests/golden/send_plan_writebatch.json) as (name, batch, case)."""
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "send_plan_writebatch.json")))
    names = sorted(g["destinations"])
    remote = []
    for nm in names:
        d = g["destinations"][nm]
        remote.append(v4(d["addr"], d["port"]) if d["family"] == 4 else v6(d["addr"], d["port"]))
    out = []
    for cs in g["cases"]:
        b = batch([(s, names.index(d)) for s, d in zip(cs["sizes"], cs["dst"])], remote=remote, via=None,
                  socket_v4=g["writer"]["socket_v4"], max_segments=g["writer"]["max_segments"],
                  chunk_packets=g["writer"]["chunk_packets"])
        out.append((cs["name"], b, cs, names))
    return out


# ---- the models' batches and plans as the ABI's arrays ---------------------------------------------

def arrays(b: M.Batch):
    """(wires, wire_status, packets, via or None, remote) as numpy arrays of the ABI's types."""
    n = len(b.lens)
    wires = np.zeros(n, I.TX_WIRE_DTYPE)
    wires["out_off"] = np.array(b.out_off, np.uint64)
    wires["counter"] = np.arange(n, dtype=np.uint64) + 1
    wires["len"] = np.array(b.lens, np.uint32)
    wires["packet"] = np.array(b.packet, np.uint32)
    wires["reserved"] = np.array(b.flags, np.uint32)
    packets = np.zeros(len(b.pkt_tunnel), I.TX_PACKET_DTYPE)
    packets["tunnel"] = np.array(b.pkt_tunnel, np.uint32)
    remote = np.zeros(len(b.remote), L.UDP_ADDR_DTYPE)
    for t, (fam, addr, port, res) in enumerate(b.remote):
        remote[t]["addr"] = np.frombuffer(addr, np.uint8)
        remote[t]["port"], remote[t]["family"], remote[t]["reserved"] = port, fam, res
    via = None
    if b.via is not None:
        via = np.zeros(len(b.via), L.RELAY_ROUTE_DTYPE)
        via["tunnel"] = np.array(b.via, np.uint32)
    return wires, np.array(b.status, np.int32), packets, via, remote


def plan_arrays(p: M.Plan):
    """A model's plan as (iov, entries, wire_entry, send_status) arrays of the ABI's types."""
    iov = np.zeros(len(p.iov), L.SEND_IOV_DTYPE)
    for k, (off, ln, w) in enumerate(p.iov):
        iov[k] = (off, ln, w)
    ent = np.zeros(len(p.entries), L.SEND_ENTRY_DTYPE)
    for k, e in enumerate(p.entries):
        ent[k] = e
    return iov, ent, np.array(p.wire_entry, np.uint32), np.array(p.send_status, np.int32)


def host_plan(b: M.Batch) -> M.Plan:
    """neb_tx_send_plan_host over the batch, as a model's Plan."""
    wires, st, packets, via, remote = arrays(b)
    r = I.send_plan_host(wires, st, packets, via, remote, b.socket_v4, b.max_segments, b.chunk_packets)
    return M.Plan([tuple(int(x) for x in v) for v in r.iov.tolist()], [tuple(int(x) for x in e) for e in r.entries.tolist()],
                  [int(x) for x in r.wire_entry], [int(x) for x in r.send_status])


def sized(n: int, seed: int, **kw) -> M.Batch:
    """Exactly n wires: runs of falling and equal lengths to a few destinations, some unroutable, some
    NOT_SENT, a bad index now and then."""
    rng = random.Random(seed)
    pool = [A, B, A_PORT, BAD6, MAPPED, RELAY, TARGET, A_TWIN]
    wires, ln, dst = [], 1200, A
    while len(wires) < n:
        r = rng.random()
        if r < 0.04:
            dst = rng.choice(pool)
        if r < 0.08:
            ln = rng.choice([1332, 1200, 600, 100, 32500, 21667, 0, 65001])
        elif r < 0.2:
            ln = max(ln - rng.randrange(1, 4), 1)
        t = dst if rng.random() > 0.01 else len(REMOTE) + 1
        wires.append((ln, t, NS if rng.random() < 0.05 else OK, M.WIRE_VIA if dst == TARGET else 0))
    return batch(wires, **kw)
