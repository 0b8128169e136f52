"""Directed cases of the RX receive plan at the edges of its rules and of the device form's geometry,
shared by the CPU tests (tests/test_recv_plan_cases.py), the host ABI test and the GPU test. Every
case states a condition (`reaches`) over the model's plan, so that a case which no longer reaches its
edge fails instead of passing vacuously. Every case carries both inputs of the segment size: the
control slot (used with d_ctrl) and neb_recv_entry.seg_size (used without); `decoy` cases give the
two different sizes on purpose.
"""
from __future__ import annotations

import ipaddress
import json
import os
import random
import struct
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np

import recv_plan_ref as M
from nebula_amd import _lib as L

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
IPPROTO_IP, IP_TOS = 0, 1
FILLER = 0xEE  # the bytes of a control slot that no cmsg covers


# ---- sockaddrs and control messages ------------------------------------------------------------------

def sockaddr4(ip: str, port: int = 4242, family: int = 2, junk: int = 0) -> bytes:
    """sockaddr_in in msg_name's 28 bytes; `junk` fills sin_zero and the bytes behind it."""
    return struct.pack("<H", family) + struct.pack(">H", port) + ipaddress.IPv4Address(ip).packed + bytes([junk]) * 20


def sockaddr6(ip, port: int = 4242, family: int = 10, junk: int = 0) -> bytes:
    """sockaddr_in6; `junk` fills sin6_flowinfo and sin6_scope_id."""
    raw = ip if isinstance(ip, bytes) else ipaddress.IPv6Address(ip).packed
    return struct.pack("<H", family) + struct.pack(">H", port) + bytes([junk]) * 4 + raw + bytes([junk]) * 4


def cmsg(level: int, typ: int, data: bytes, clen: Optional[int] = None, space: Optional[int] = None) -> bytes:
    """One control message: header, data, padding to CmsgSpace. clen overrides cmsg_len (as u64)."""
    n = M.SIZEOF_CMSGHDR + len(data) if clen is None else clen
    body = struct.pack("<Qii", n & (2**64 - 1), level, typ) + data
    space = M.SIZEOF_CMSGHDR + M.align8(len(data)) if space is None else space
    return body[:space] + b"\0" * (space - len(body))


def gro(size: int) -> bytes:
    return cmsg(M.SOL_UDP, M.UDP_GRO, struct.pack("<i", size))


A4 = sockaddr4("192.0.2.1")


def entry(length: int, seg: int = 0, off: int = 0, name: bytes = A4, ctrl: Optional[bytes] = None,
          ctrl_len: Optional[int] = None, decoy: Optional[int] = None) -> M.Entry:
    """ctrl None: the slot holds UDP_GRO = seg (nothing when seg == 0). decoy: seg_size when it is to differ."""
    if ctrl is None:
        ctrl = gro(seg) if seg != 0 else b""
    return M.Entry(off=off, len=length, seg=seg if decoy is None else decoy, name=name, ctrl=ctrl,
                   ctrl_len=len(ctrl) if ctrl_len is None else ctrl_len)


def batch(entries: List[M.Entry], socket_v4: bool = True, ctrl_stride: int = 64,
          max_packets: Optional[int] = None, lay_out: bool = True) -> M.Batch:
    """Pads every control slot to the stride with FILLER; lays the buffers out one after the other
    (64-byte slots' worth apart at least) unless the entries carry offsets of their own."""
    at = 0
    for e in entries:
        assert len(e.ctrl) <= ctrl_stride
        e.ctrl = e.ctrl + bytes([FILLER]) * (ctrl_stride - len(e.ctrl))
        if lay_out and e.off == 0:
            e.off = at
            at += (min(e.len, 1 << 20) + 63) & ~63
    return M.Batch(entries=entries, socket_v4=socket_v4, ctrl_stride=ctrl_stride, max_packets=max_packets)


@dataclass
class Case:
    name: str
    batch: M.Batch
    reaches: Callable  # (plan with d_ctrl, plan with seg_size) -> bool
    same: bool = True  # both modes give the same plan


def lens(p: M.Plan, j: int) -> List[int]:
    """The packet lengths of entry j."""
    return [p.pk[i][1] for i in range(len(p.pk)) if p.pkt_entry[i] == j]


# ---- sizes -------------------------------------------------------------------------------------------

def _size_cases():
    out = []
    n = 1400
    for name, seg, want in (("seg_len_minus_1", n - 1, [n - 1, 1]), ("seg_eq_len", n, [n]), ("seg_len_plus_1", n + 1, [n]),
                            ("seg_int32_min", INT32_MIN, [n]), ("seg_minus_1", -1, [n]), ("seg_0", 0, [n]),
                            ("seg_1", 1, [1] * n), ("seg_int32_max", INT32_MAX, [n])):
        b = batch([entry(n, seg), entry(100, 0)])
        out.append(Case(name, b, lambda c, s, want=want: lens(c, 0) == want and c.entry_first == [0, len(want)]))
    for seg in (INT32_MIN, -1, 0, 1, INT32_MAX):
        b = batch([entry(0, seg, off=4096), entry(100, 0, off=8192)])
        out.append(Case(f"len_0_seg_{seg}", b, lambda c, s: c.pk[0] == (4096, 0) and c.entry_first == [0, 1] and c.npackets == 2))
    return out


# ---- width -------------------------------------------------------------------------------------------

def _width_cases():
    out = []
    # ceil's numerator len + seg - 1 passes 2^32, and the second packet's offset crosses a multiple of 2^32.
    # (2 * 0x7FFFFFFF > 0xFFFFFFF0: the entry holds two packets, k * seg itself never reaches 2^32.)
    off = (1 << 40) - 5
    b = batch([entry(0xFFFFFFF0, 0x7FFFFFFF, off=off), entry(9, 0, off=77)], lay_out=False)
    out.append(Case("width_numerator_past_32_bits", b,
                    lambda c, s: c.pk[:2] == [(off, 0x7FFFFFFF), (off + 0x7FFFFFFF, 0x7FFFFFF1)] and c.entry_first == [0, 2]
                    and 0xFFFFFFF0 + 0x7FFFFFFF - 1 >= 1 << 32 and (off >> 32) != ((off + 0x7FFFFFFF) >> 32)))
    small = [entry(10, 0, off=64 * (k + 1)) for k in range(5)]
    big = lambda: entry(0xFFFFFFFF, 1, off=1 << 33)  # noqa: E731
    b = batch([big()] + [entry(10, 0, off=64 * (k + 1)) for k in range(5)], max_packets=9, lay_out=False)
    out.append(Case("width_big_entry_first_is_cut", b,
                    lambda c, s: c.count[0] == 0xFFFFFFFF and sum(c.count) >= 1 << 32 and (c.npackets, c.done) == (0, 0)
                    and c.entry_first == [M.NONE] * 6))
    b = batch(small + [big(), entry(10, 0, off=999)], max_packets=9, lay_out=False)
    out.append(Case("width_small_entries_then_big", b,
                    lambda c, s: sum(c.count) >= 1 << 32 and (c.npackets, c.done) == (5, 5)
                    and c.entry_first == [0, 1, 2, 3, 4, M.NONE, M.NONE]))
    return out


# ---- geometry ----------------------------------------------------------------------------------------

def ones(n: int, at: int = 0) -> List[M.Entry]:
    """n one-packet entries of differing lengths and sources."""
    return [entry(60 + (at + k) % 1300, 0, name=sockaddr4(f"10.{(at + k) >> 16 & 255}.{(at + k) >> 8 & 255}.{(at + k) & 255}",
                                                          1024 + (at + k) % 60000)) for k in range(n)]


def _geometry_cases():
    out = []
    for n in (1, 255, 256, 257, 5000, 70000):
        out.append(Case(f"entries_{n}", batch(ones(n)),
                        lambda c, s, n=n: (c.npackets, c.done) == (n, n) and c.entry_first[-1] == n - 1))
    b = batch([entry(255 * 20, 20), entry(33, 0), entry(34, 0), entry(35 * 3, 35), entry(36, 0)])
    out.append(Case("boundaries_at_255_256_257", b, lambda c, s: c.entry_first == [0, 255, 256, 257, 260]))
    for where, k in (("first", 0), ("middle", 300), ("last", 600)):
        es = ones(600)
        es.insert(k, entry(65535, 1, name=sockaddr4("198.51.100.7", 0x0102)))
        out.append(Case(f"entry_of_65535_{where}", batch(es, max_packets=65535 + 600 + 300),
                        lambda c, s, k=k: c.count[k] == 65535 and c.npackets == 65535 + 600 and c.entry_first[k] == k
                        and (k == 600 or c.entry_first[k + 1] == k + 65535)))
    return out


# ---- capacity ----------------------------------------------------------------------------------------

def _capacity_entries():
    es = []
    for k in range(121):
        es.append(entry(1364 * (1 + k % 7) - (k % 3) * 100, 1364 if k % 7 else 0))
    return es


def _capacity_cases():
    out = []
    total = sum(M.segment_count(e.len, e.seg) for e in _capacity_entries())
    boundary = sum(M.segment_count(e.len, e.seg) for e in _capacity_entries()[:70])
    assert total > 256 + 121
    for name, mp, want in (("total", total, (total, 121)), ("total_minus_1", total - 1, None), ("total_plus_1", total + 1, (total, 121)),
                           ("total_plus_300", total + 300, (total, 121)), ("entry_boundary", boundary, (boundary, 70)),
                           ("zero", 0, (0, 0))):
        b = batch(_capacity_entries(), max_packets=mp)
        if want is None:
            reach = lambda c, s: c.done == 120 and c.entry_first[-1] == M.NONE and c.npackets < c.max_packets  # noqa: E731
        else:
            reach = lambda c, s, want=want: (c.npackets, c.done) == want  # noqa: E731
        out.append(Case(f"max_packets_{name}", b, reach))
    b = batch(ones(3), max_packets=3 + 700)
    out.append(Case("padding_over_several_workgroups", b, lambda c, s: c.max_packets - c.npackets > 2 * 256))
    b = batch([], max_packets=300)
    out.append(Case("no_entries", b, lambda c, s: (c.npackets, c.done) == (0, 0) and c.max_packets == 300))
    b = batch([], max_packets=0)
    out.append(Case("no_entries_no_slots", b, lambda c, s: (c.npackets, c.done, c.max_packets) == (0, 0, 0)))
    return out


# ---- sources -----------------------------------------------------------------------------------------

def mapped(ip4: str, flip: Optional[int] = None, bit: int = 0) -> bytes:
    """::ffff:a.b.c.d as 16 bytes, one bit of byte `flip` toggled."""
    raw = bytearray(b"\0" * 10 + b"\xff\xff" + ipaddress.IPv4Address(ip4).packed)
    if flip is not None:
        raw[flip] ^= 1 << bit
    return bytes(raw)


def _source_cases():
    out = []
    b = batch([entry(100, 0, name=sockaddr4("192.0.2.1", 0x0102)), entry(100, 0, name=sockaddr4("203.0.113.9", 0x0201)),
               entry(300, 100, name=sockaddr4("192.0.2.1", 0x0102, family=0xBEEF, junk=0xCC))], socket_v4=True)
    out.append(Case("v4_socket_ports_and_garbage", b,
                    lambda c, s: [f[2] for f in c.frm] == [0x0102, 0x0201, 0x0102] and c.frm[0] == c.frm[2]
                    and c.frm[0] == (4, bytes([192, 0, 2, 1]) + b"\0" * 12, 0x0102) and len(c.src) == 5))
    names = [sockaddr6("2001:db8::1", 0x0102), sockaddr6(mapped("10.1.2.3"), 0x0201),
             sockaddr6(mapped("10.1.2.3", 9), 7), sockaddr6(mapped("10.1.2.3", 10), 7), sockaddr6(mapped("10.1.2.3", 11, 7), 7),
             sockaddr6(mapped("10.1.2.3", 0, 7), 7), sockaddr6(mapped("10.1.2.3"), 0x0201, family=0, junk=0x5A)]
    b = batch([entry(200, 100, name=nm) for nm in names], socket_v4=False)
    out.append(Case("v6_socket_unmap_and_neighbours", b,
                    lambda c, s: [f[0] for f in c.frm] == [6, 4, 6, 6, 6, 6, 4] and c.frm[1] == c.frm[6]
                    and c.frm[1][1] == bytes([10, 1, 2, 3]) + b"\0" * 12 and c.frm[2][1][9] == 1 and c.frm[3][1][10] == 0xFE
                    and c.frm[4][1][11] == 0x7F and c.src[2] == (4, c.frm[1][1])))
    return out


# ---- control buffers ---------------------------------------------------------------------------------

def _ctrl_cases():
    out = []
    n = 3000

    def one(name, ctrl, want_seg, ctrl_len=None, stride=64, same=False):
        b = batch([entry(n, 7, ctrl=ctrl, ctrl_len=ctrl_len), entry(50, 0)], ctrl_stride=stride)
        out.append(Case("ctrl_" + name, b, lambda c, s: c.seg[0] == want_seg and s.seg[0] == 7
                        and c.count[0] == M.segment_count(n, want_seg), same=same))

    tos = cmsg(IPPROTO_IP, IP_TOS, b"\x2e")  # len 17, advance 24
    assert len(tos) == 24
    one("len_0", gro(1000), 0, ctrl_len=0)
    one("len_15", gro(1000), 0, ctrl_len=15)
    one("gro_alone", gro(1000), 1000)
    one("gro_after_tos", tos + gro(1000), 1000)
    one("two_gro_last_wins", gro(1000) + gro(1500), 1500)
    one("right_level_wrong_type", cmsg(M.SOL_UDP, 103, struct.pack("<i", 1000)), 0)
    one("wrong_level_right_type", cmsg(6, M.UDP_GRO, struct.pack("<i", 1000)), 0)
    # a UDP_GRO cmsg of the header alone (len 16) 18 bytes before L: its 4 data bytes would end 2 past L
    one("gro_data_past_the_end", gro(1000) + cmsg(M.SOL_UDP, M.UDP_GRO, struct.pack("<i", 1500), clen=16)[:18], 1000,
        ctrl_len=24 + 18)
    one("negative_payload", gro(-1400), -1400)
    one("ctrl_len_above_stride", gro(1000), 1000, ctrl_len=4096, stride=24)
    one("gro_just_past_ctrl_len", gro(1000) + gro(1500), 1000, ctrl_len=24)
    for name, clen in (("cmsg_len_15", 15), ("cmsg_len_rest_plus_1", 48 - 24 + 1), ("cmsg_len_2_63_minus_8", (1 << 63) - 8),
                       ("cmsg_len_2_63", 1 << 63)):
        bad = cmsg(M.SOL_UDP, M.UDP_GRO, struct.pack("<i", 1500), clen=clen)
        one(name, gro(1000) + bad, 1000, ctrl_len=48)
    return out


def directed() -> List[Case]:
    return _size_cases() + _width_cases() + _geometry_cases() + _capacity_cases() + _source_cases() + _ctrl_cases()


# ---- random batches ----------------------------------------------------------------------------------

def random_batches(seed: int, count: int, nmax: int = 40):
    rng = random.Random(seed)
    for _ in range(count):
        v4 = rng.random() < 0.5
        stride = rng.choice([24, 32, 64, 128])
        es = []
        for _ in range(rng.randrange(0, nmax)):
            length = rng.choice([0, 1, 17, 1364, rng.randrange(0, 65536), rng.randrange(0, 5000)])
            seg = rng.choice([0, 0, 1364, rng.randrange(-3, 20), rng.randrange(1, 3000), length, length + 1, max(length - 1, 0)])
            if length > 4000 and 0 < seg < 40:
                seg += 40  # keep the model's packet lists short
            raw = bytes(rng.randrange(256) for _ in range(16))
            if rng.random() < 0.4:
                raw = mapped("10.0.0.%d" % rng.randrange(256), rng.choice([None, None, 9, 10, 11]), rng.randrange(8))
            nm = sockaddr4("10.0.%d.%d" % (rng.randrange(256), rng.randrange(256)), rng.randrange(65536), junk=rng.randrange(256)) \
                if v4 else sockaddr6(raw, rng.randrange(65536), junk=rng.randrange(256))
            r = rng.random()
            if r < 0.5:
                ctrl, clen = None, None
            elif r < 0.75:
                ctrl = (cmsg(IPPROTO_IP, IP_TOS, b"\1") + gro(seg))[:stride]
                clen = rng.choice([None, rng.randrange(0, stride + 9)])
            else:
                ctrl = bytes(rng.choice([0, 0, 16, 17, 20, 24, 104, 255, rng.randrange(256)]) for _ in range(stride))
                clen = rng.randrange(0, stride + 9)
            es.append(entry(length, seg, name=nm, ctrl=ctrl, ctrl_len=clen,
                            decoy=rng.choice([None, None, rng.randrange(-2, 2000)])))
        b = batch(es, socket_v4=v4, ctrl_stride=stride)
        total = max(sum(M.listen_out(b, True).count), sum(M.listen_out(b, False).count))
        b.max_packets = rng.choice([total, 0, total + rng.randrange(0, 300), rng.randrange(0, total + 2)])
        yield b


# ---- the reference tests' own tables -----------------------------------------------------------------

def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recv_plan_deliver.json")) as f:
        return json.load(f)


# ---- numpy forms -------------------------------------------------------------------------------------

def arrays(b: M.Batch):
    """(entries as RECV_ENTRY_DTYPE, the control slots as uint8 of nentries * ctrl_stride)."""
    n = len(b.entries)
    en = np.zeros(n, L.RECV_ENTRY_DTYPE)
    ctrl = np.zeros(n * b.ctrl_stride, np.uint8)
    for j, e in enumerate(b.entries):
        en[j] = (e.off, e.len, e.seg, np.frombuffer(e.name, np.uint8), e.ctrl_len)
        ctrl[j * b.ctrl_stride:(j + 1) * b.ctrl_stride] = np.frombuffer(e.ctrl, np.uint8)
    return en, ctrl


def plan_arrays(p: M.Plan, nentries: int):
    """The six outputs as the call writes them, padding included: pk, src, pkt_entry over max_packets
    slots, from and entry_first over the entries, counts."""
    mp = p.max_packets
    pk = np.zeros(mp, L.RX_PACKET_DTYPE)
    pk["key_id"] = L.KEYS_MIXED
    src = np.zeros(mp, L.RX_SOURCE_DTYPE)
    pe = np.full(mp, L.RECV_NONE, np.uint32)
    k = p.npackets
    if k:
        pk["off"][:k] = [x[0] for x in p.pk]
        pk["len"][:k] = [x[1] for x in p.pk]
        src["family"][:k] = [x[0] for x in p.src]
        src["addr"][:k] = np.frombuffer(b"".join(x[1] for x in p.src), np.uint8).reshape(k, 16)
        pe[:k] = p.pkt_entry
    frm = np.zeros(nentries, L.UDP_ADDR_DTYPE)
    if nentries:
        frm["family"] = [x[0] for x in p.frm]
        frm["addr"] = np.frombuffer(b"".join(x[1] for x in p.frm), np.uint8).reshape(nentries, 16)
        frm["port"] = [x[2] for x in p.frm]
    first = np.array(p.entry_first, np.uint32)
    return pk, src, pe, frm, first, np.array([p.npackets, p.done], np.uint32)


OUT_ITEMS = (("pk", 16), ("src", 20), ("pkt_entry", 4), ("from", 20), ("entry_first", 4))
FILL = 0xA5


def host_plan(b: M.Batch, use_ctrl: bool, max_packets: int, slack: int = 0, optional: bool = True):
    """neb_rx_recv_plan_host over FILL-initialised outputs with `slack` elements beyond each array.
    Returns (rc, {name: raw bytes}, counts)."""
    import ctypes as C

    en, ctrl = arrays(b)
    n = len(en)
    size = {"pk": max_packets, "src": max_packets, "pkt_entry": max_packets, "from": n, "entry_first": n}
    out = {name: np.full((size[name] + slack) * item, FILL, np.uint8) for name, item in OUT_ITEMS}
    counts = np.full(2, 0xDEADBEEF, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    opt = lambda a: vp(a) if optional else None  # noqa: E731
    rc = L.lib().neb_rx_recv_plan_host(vp(en), n, vp(ctrl) if use_ctrl else None, b.ctrl_stride, int(b.socket_v4),
                                       vp(out["pk"]), opt(out["src"]), opt(out["pkt_entry"]), max_packets, opt(out["from"]),
                                       vp(out["entry_first"]), vp(counts))
    return rc, out, counts


def compare(out, counts, want, slack: int, optional: bool = True):
    """Byte for byte over [0, max_packets) / [0, nentries); FILL beyond; optional outputs untouched when NULL."""
    w = dict(zip([n for n, _ in OUT_ITEMS], want[:5]))
    assert counts.tolist() == want[5].tolist(), ("counts", counts.tolist(), want[5].tolist())
    for name, item in OUT_ITEMS:
        got = np.asarray(out[name])
        if not optional and name in ("src", "pkt_entry", "from"):
            assert (got == FILL).all(), name
            continue
        nb = w[name].nbytes
        if got[:nb].tobytes() != w[name].tobytes():
            bad = np.nonzero(got[:nb] != w[name].view(np.uint8).reshape(-1))[0]
            raise AssertionError(f"{name}: first difference at element {bad[0] // item} of {nb // item}")
        assert got.size == nb + slack * item and (got[nb:] == FILL).all(), name + " beyond"
