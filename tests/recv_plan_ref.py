"""A model of the RX receive plan (neb_rx_recv_plan, include/nebula_aead.h), written from its stated
semantics: literal and sequential, one function per function of the reference's receive loop
(udp/udp_linux.go:237-331, read as text): get_from, parse_recv_cmsg, deliver_segments, and listen_out,
which is the loop over the entries with the call's capacity rule on top.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

NONE = 0xFFFFFFFF
SIZEOF_CMSGHDR = 16  # Linux LP64: {u64 len; i32 level; i32 type}
SOL_UDP, UDP_GRO = 17, 104
MAPPED_PREFIX = b"\0" * 10 + b"\xff\xff"


@dataclass
class Entry:
    off: int
    len: int
    seg: int = 0           # neb_recv_entry.seg_size: used when the call gets no control buffers
    name: bytes = b"\0" * 28
    ctrl: bytes = b""      # the entry's control slot, as many bytes as the test wants to exist there
    ctrl_len: int = 0      # msg_controllen after the call


@dataclass
class Batch:
    entries: List[Entry]
    socket_v4: bool = True
    ctrl_stride: int = 64
    max_packets: Optional[int] = None  # None: exactly the packets of all entries


@dataclass
class Plan:
    pk: List[Tuple[int, int]] = field(default_factory=list)       # (off, len) per emitted packet
    src: List[Tuple[int, bytes]] = field(default_factory=list)    # (family, 16 address bytes) per emitted packet
    pkt_entry: List[int] = field(default_factory=list)
    frm: List[Tuple[int, bytes, int]] = field(default_factory=list)  # (family, address, port) per entry
    entry_first: List[int] = field(default_factory=list)
    seg: List[int] = field(default_factory=list)                  # per entry: the size that was used
    count: List[int] = field(default_factory=list)                # per entry: its packets (NONE entries too)
    npackets: int = 0
    done: int = 0
    max_packets: int = 0


def get_from(name: bytes, is_v4: bool) -> Tuple[int, bytes, int]:
    """(family, the address in 16 bytes with the unused ones zero, port)."""
    port = struct.unpack(">H", name[2:4])[0]
    if is_v4:
        return 4, name[4:8] + b"\0" * 12, port
    ip = name[8:24]
    if ip[:12] == MAPPED_PREFIX:  # Unmap
        return 4, ip[12:16] + b"\0" * 12, port
    return 6, ip, port


def align8(n: int) -> int:
    return (n + 7) & ~7


def parse_recv_cmsg(ctrl: bytes) -> int:
    """The UDP_GRO size in ctrl (already cut to the bytes that may be read), or 0."""
    gso = 0
    off = 0
    while off + SIZEOF_CMSGHDR <= len(ctrl):
        clen, level, typ = struct.unpack_from("<qii", ctrl, off)  # len as a signed int
        if clen < SIZEOF_CMSGHDR or clen > len(ctrl) - off:
            return gso
        data_off = off + SIZEOF_CMSGHDR
        if level == SOL_UDP and typ == UDP_GRO and data_off + 4 <= len(ctrl):
            gso = struct.unpack_from("<i", ctrl, data_off)[0]
        off += SIZEOF_CMSGHDR + align8(clen - SIZEOF_CMSGHDR)
    return gso


def segment_count(length: int, seg: int) -> int:
    if seg <= 0 or seg >= length:
        return 1
    return -(-length // seg)


def deliver_segments(off: int, length: int, seg: int):
    """Yields (off, len) of every delivered packet."""
    if seg <= 0 or seg >= length:
        yield off, length
        return
    at = 0
    while at < length:
        end = min(at + seg, length)
        yield off + at, end - at
        at += seg


def seg_size(e: Entry, use_ctrl: bool, ctrl_stride: int) -> int:
    if not use_ctrl:
        return e.seg
    L = min(e.ctrl_len, ctrl_stride)
    assert len(e.ctrl) >= L
    return parse_recv_cmsg(e.ctrl[:L])


def listen_out(b: Batch, use_ctrl: bool) -> Plan:
    p = Plan()
    first = 0
    cut = False
    for j, e in enumerate(b.entries):
        s = seg_size(e, use_ctrl, b.ctrl_stride)
        c = segment_count(e.len, s)
        p.seg.append(s)
        p.count.append(c)
        p.frm.append(get_from(e.name, b.socket_v4))
    total = sum(p.count)
    p.max_packets = total if b.max_packets is None else b.max_packets
    for j, e in enumerate(b.entries):
        c = p.count[j]
        if cut or first + c > p.max_packets:
            cut = True
            p.entry_first.append(NONE)
            continue
        p.entry_first.append(first)
        fam, addr, _ = p.frm[j]
        for pk in deliver_segments(e.off, e.len, p.seg[j]):
            p.pk.append(pk)
            p.src.append((fam, addr))
            p.pkt_entry.append(j)
        first += c
        assert len(p.pk) == first
        p.done = j + 1
    p.npackets = first
    return p
