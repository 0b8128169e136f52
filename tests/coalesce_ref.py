"""TEST INFRASTRUCTURE ONLY: the sequential model of the receive path between the open and the TUN
write, for tests/test_rx_coalesce.py and tests/test_gpu_rx_coalesce.py.

A pure-Python restatement, packet by packet, of slackhq/nebula (read as text, not copied):
  newPacket / parseV4 / parseV6      outside.go:320-472
  IPv6FindUpperProtocol              iputil/packet.go:349-395
  MultiCoalescer Commit/dispatch/Flush   overlay/batch/multi_coalesce.go:67-133
  flowKey.parseIPAt, ipHeadersMatch, ipv4CanCoalesceID   overlay/batch/coalesce_core.go:42-138
  TCPCoalescer                       overlay/batch/tcp_coalesce.go:103-472
  UDPCoalescer                       overlay/batch/udp_coalesce.go:87-345
  Passthrough                        overlay/batch/passthrough.go:21-38
  Offload.Write / WriteGSO           overlay/tio/tio_gso_linux.go:49-55, :280-291, :325-404
and builders of IPv4 / IPv6 x TCP / UDP / ICMP packets with valid checksums. The product never
imports this module.
"""
from __future__ import annotations

import struct

TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
FIN, SYN, RST, PSH, ACK, URG, ECE, CWR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
F_NEEDS_CSUM, F_DATA_VALID = 1, 2
GSO_NONE, GSO_TCPV4, GSO_TCPV6, GSO_UDP_L4 = 0, 1, 4, 5
LANE_TCP, LANE_UDP, LANE_PT = 0, 1, 2
COALESCE_TCP, COALESCE_UDP = 1, 2
PLAIN_PARSED, PLAIN_FRAG_ANY, PLAIN_SKIP = 1, 2, 4
ST_OK, ST_INVALID, ST_NO_SPACE, ST_SKIP = 0, 5, 6, 7
WRITE_NONE = 0xFFFFFFFF
MAX_SEGS = 64       # tcpCoalesceMaxSegs / udpCoalesceMaxSegs
BUF_SIZE = 65535    # tcpCoalesceBufSize / udpCoalesceBufSize


# ---- packet builders -------------------------------------------------------------------------------
def csum16(b: bytes, init: int = 0) -> int:
    if len(b) & 1:
        b = b + b"\0"
    s = init + sum(struct.unpack(f">{len(b) // 2}H", b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def ip4(s: str) -> bytes:
    return bytes(int(x) for x in s.split("."))


def ip6(n: int) -> bytes:
    return (0xFD00 << 112 | n).to_bytes(16, "big")


def ipv4(src, dst, proto, payload, *, ident=0, df=True, tos=0, ttl=64, options=b"", frag_off=0, mf=False):
    ihl = 20 + len(options)
    assert ihl % 4 == 0
    ff = (0x4000 if df else 0) | (0x2000 if mf else 0) | frag_off
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl // 4, tos, ihl + len(payload), ident, ff, ttl, proto, 0,
                              src, dst) + options)
    struct.pack_into(">H", h, 10, ~csum16(h) & 0xFFFF)
    return bytes(h) + payload


def ipv6(src, dst, nh, payload, *, tc=0, flow=0, hlim=64):
    """payload: everything after the fixed header (extension headers included); nh: first next header."""
    return struct.pack(">IHBB16s16s", 6 << 28 | tc << 20 | flow, len(payload), nh, hlim, src, dst) + payload


def _pseudo(src, dst, proto, l4len):
    if len(src) == 4:
        return csum16(src + dst + struct.pack(">HH", proto, l4len))
    return csum16(src + dst + struct.pack(">II", l4len, proto))


def tcp_hdr(src, dst, sport, dport, seq, payload, flags=ACK, *, ack=1, window=1000, options=b""):
    off = 20 + len(options)
    assert off % 4 == 0
    h = bytearray(struct.pack(">HHIIBBHHH", sport, dport, seq & 0xFFFFFFFF, ack, off // 4 << 4, flags, window, 0, 0)
                  + options)
    c = ~csum16(bytes(h) + payload, _pseudo(src, dst, TCP, off + len(payload))) & 0xFFFF
    struct.pack_into(">H", h, 16, c)
    return bytes(h) + payload


def udp_hdr(src, dst, sport, dport, payload):
    h = bytearray(struct.pack(">HHHH", sport, dport, 8 + len(payload), 0))
    c = ~csum16(bytes(h) + payload, _pseudo(src, dst, UDP, 8 + len(payload))) & 0xFFFF
    struct.pack_into(">H", h, 6, c or 0xFFFF)
    return bytes(h) + payload


def tcp4(src, dst, sport, dport, seq, payload, flags=ACK, *, tcp_kw=None, **ip_kw):
    return ipv4(src, dst, TCP, tcp_hdr(src, dst, sport, dport, seq, payload, flags, **(tcp_kw or {})), **ip_kw)


def tcp6(src, dst, sport, dport, seq, payload, flags=ACK, *, tcp_kw=None, **ip_kw):
    return ipv6(src, dst, TCP, tcp_hdr(src, dst, sport, dport, seq, payload, flags, **(tcp_kw or {})), **ip_kw)


def udp4(src, dst, sport, dport, payload, **ip_kw):
    return ipv4(src, dst, UDP, udp_hdr(src, dst, sport, dport, payload), **ip_kw)


def udp6(src, dst, sport, dport, payload, **ip_kw):
    return ipv6(src, dst, UDP, udp_hdr(src, dst, sport, dport, payload), **ip_kw)


def icmp4(src, dst, icmp_id, payload, **ip_kw):
    b = bytearray(struct.pack(">BBHHH", 8, 0, 0, icmp_id, 1) + payload)
    struct.pack_into(">H", b, 2, ~csum16(b) & 0xFFFF)
    return ipv4(src, dst, ICMP, bytes(b), **ip_kw)


def icmp6(src, dst, icmp_id, payload, **ip_kw):
    b = bytearray(struct.pack(">BBHHH", 128, 0, 0, icmp_id, 1) + payload)
    struct.pack_into(">H", b, 2, ~csum16(b, _pseudo(src, dst, ICMP6, len(b))) & 0xFFFF)
    return ipv6(src, dst, ICMP6, bytes(b), **ip_kw)


# ---- newPacket (outside.go:320-472) ------------------------------------------------------------------
def ipv6_find_upper_protocol(p: bytes):
    """iputil/packet.go:349-395 -> (proto, offset, is_fragment, any_fragment) or None (error)."""
    if len(p) < 40:
        return None
    nh, off, anyf = p[6], 40, False
    for _ in range(8):  # maxIPv6ExtHeaders
        if nh in (0, 43, 60):
            if len(p) < off + 2:
                return None
            nh, off = p[off], off + ((p[off + 1] + 1) << 3)
        elif nh == 44:
            if len(p) < off + 8:
                return None
            anyf = True
            if p[off + 2] != 0 or p[off + 3] & 0xF8:
                return p[off], off, True, anyf
            nh, off = p[off], off + 8
        elif nh == 51:
            if len(p) < off + 2:
                return None
            nh, off = p[off], off + ((p[off + 1] + 2) << 2)
        else:
            if off > len(p):
                return None
            return nh, off, False, anyf
    return nh, off, False, anyf


def new_packet(d: bytes):
    """-> (Protocol, FragAny, IPHdrLen) or None when newPacket returns an error (the packet is dropped)."""
    if len(d) < 1:
        return None
    ver = d[0] >> 4
    if ver == 4:  # parseV4, outside.go:410-472
        if len(d) < 20:
            return None
        ihl = (d[0] & 0x0F) << 2
        if ihl < 20:
            return None
        ff = struct.unpack_from(">H", d, 6)[0]
        fragment = (ff & 0x1FFF) != 0
        proto = d[9]
        min_len = ihl
        if not fragment:
            min_len += 6 if proto == ICMP else 4
        if len(d) < min_len:
            return None
        return proto, (ff & 0x3FFF) != 0, ihl
    if ver == 6:  # parseV6, outside.go:339-408
        r = ipv6_find_upper_protocol(d)
        if r is None:
            return None
        proto, off, is_frag, anyf = r
        if is_frag:
            return proto, anyf, off
        if proto == ICMP6:
            if len(d) < off + 4:
                return None
            if d[off] in (128, 129) and len(d) < off + 6:
                return None
        elif proto in (TCP, UDP):
            if len(d) < off + 4:
                return None
        return proto, anyf, off
    return None


# ---- checksum seeds (tcp_coalesce.go:421-472) --------------------------------------------------------
def ipv4_hdr_checksum(hdr: bytes) -> int:
    return ~csum16(bytes(hdr)) & 0xFFFF


def pseudo_sum_ipv4(src, dst, proto, l4len):
    return sum(struct.unpack(">4H", bytes(src) + bytes(dst))) + proto + l4len


def pseudo_sum_ipv6(src, dst, proto, l4len):
    return sum(struct.unpack(">16H", bytes(src) + bytes(dst))) + (l4len >> 16) + (l4len & 0xFFFF) + proto


def fold_once_no_invert(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


# ---- the writer: Offload.Write / WriteGSO -------------------------------------------------------------
class Writer:
    """Records every TUN write: (virtio fields, bytes, first, members, lane)."""

    def __init__(self):
        self.writes = []

    def Write(self, buf, first, lane):  # tio_gso_linux.go:280-291: validVnetHdr, the packet untouched
        self.writes.append(dict(vnet_flags=F_DATA_VALID, gso_type=GSO_NONE, hdr_len=0, gso_size=0, csum_start=0,
                                csum_offset=0, data=bytes(buf), first=first, members=[first], lane=lane))

    def WriteGSO(self, hdr, thdr, pays, tcp, first, members, lane):  # tio_gso_linux.go:325-404
        assert len(pays) > 1 and all(len(p) == len(pays[0]) for p in pays[:-1]) and 0 < len(pays[-1]) <= len(pays[0])
        ver = hdr[0] >> 4
        gso_type = (GSO_TCPV4 if ver == 4 else GSO_TCPV6) if tcp else GSO_UDP_L4
        data = bytes(hdr) + bytes(thdr) + b"".join(pays)
        assert len(data) <= 65535
        self.writes.append(dict(vnet_flags=F_NEEDS_CSUM, gso_type=gso_type, hdr_len=len(hdr) + len(thdr),
                                gso_size=len(pays[0]), csum_start=len(hdr), csum_offset=16 if tcp else 6, data=data,
                                first=first, members=list(members), lane=lane))


# ---- the lanes ---------------------------------------------------------------------------------------
class _Slot:
    pass


def _parse_ip_at(pkt, ip_hdr_len):
    """flowKey.parseIPAt (coalesce_core.go:42-94) -> (trimmed, src16, dst16, is_v6) or None."""
    if len(pkt) < 20:
        return None
    ver = pkt[0] >> 4
    if ver == 4:
        if ip_hdr_len != 20 or (pkt[0] & 0x0F) * 4 != 20:
            return None
        if struct.unpack_from(">H", pkt, 6)[0] & 0x3FFF:
            return None
        total = struct.unpack_from(">H", pkt, 2)[0]
        if total > len(pkt) or total < 20:
            return None
        return pkt[:total], pkt[12:16] + bytes(12), pkt[16:20] + bytes(12), False
    if ver == 6:
        if ip_hdr_len != 40 or len(pkt) < 40:
            return None
        pl = struct.unpack_from(">H", pkt, 4)[0]
        if 40 + pl > len(pkt):
            return None
        return pkt[:40 + pl], pkt[8:24], pkt[24:40], True
    return None


def _ip_headers_match(a, b, v6):  # coalesce_core.go:104-114
    if v6:
        return a[:4] == b[:4] and a[6:40] == b[6:40]
    return a[:2] == b[:2] and a[6:10] == b[6:10] and a[12:20] == b[12:20]


def _ipv4_can_coalesce_id(seed, nxt, seg):  # coalesce_core.go:132-138
    if seed[6] & 0x40:
        return True
    return struct.unpack_from(">H", nxt, 4)[0] == (struct.unpack_from(">H", seed, 4)[0] + seg) & 0xFFFF


class _Coalescer:
    """What TCPCoalescer and UDPCoalescer share: slots in creation order, open chains by flow key."""
    tcp = False

    def __init__(self, lane):
        self.lane = lane
        self.slots = []
        self.open = {}

    def seal_all_open(self):
        self.open.clear()

    def seal_flow(self, fk):
        self.open.pop(fk, None)

    def add_verbatim(self, idx, pkt):
        s = _Slot()
        s.verbatim, s.raw, s.first, s.members = True, pkt, idx, [idx]
        self.slots.append(s)

    def commit_staged(self, idx, pkt, frag_any, ip_hdr_len):  # tcp_coalesce.go:164-177, udp_coalesce.go:129-142
        info = None if frag_any else self.parse_at(pkt, ip_hdr_len)
        if info is None:
            self.seal_all_open()
            self.add_verbatim(idx, pkt)
            return
        self.commit_parsed(idx, pkt, info)

    def seed(self, idx, pkt, info):  # tcp_coalesce.go:263-295, udp_coalesce.go:217-242
        if info["hdr_len"] + info["pay_len"] > BUF_SIZE:
            self.seal_flow(info["fk"])
            self.add_verbatim(idx, pkt)
            return
        s = _Slot()
        s.verbatim, s.raw, s.first, s.members = False, pkt, idx, [idx]
        s.hdr = bytearray(pkt[:info["hdr_len"]])  # the superpacket header; the model patches a copy
        s.hdr_len, s.ip_hdr_len, s.v6, s.fk = info["hdr_len"], info["ip_hdr_len"], info["v6"], info["fk"]
        s.gso = s.total_pay = info["pay_len"]
        s.nseg = 1
        s.next_seq = (info.get("seq", 0) + info["pay_len"]) & 0xFFFFFFFF
        s.pays = [pkt[info["hdr_len"]:info["hdr_len"] + info["pay_len"]]]
        self.slots.append(s)
        if self.tcp and info["flags"] & PSH:
            self.seal_flow(info["fk"])
        else:
            self.open[info["fk"]] = s

    def commit_data(self, idx, pkt, info):  # tcp_coalesce.go:206-227, udp_coalesce.go:155-176
        s = self.open.get(info["fk"])
        if s is not None:
            if self.can_append(s, pkt, info):
                if self.append_payload(s, idx, pkt, info):
                    self.seal_flow(info["fk"])
                return
            self.seal_flow(info["fk"])
        self.seed(idx, pkt, info)

    def can_append_common(self, s, pkt, info):
        if info["hdr_len"] != s.hdr_len:
            return False
        if self.tcp and info["seq"] != s.next_seq:
            return False
        if s.nseg >= MAX_SEGS:
            return False
        if info["pay_len"] > s.gso:
            return False
        if s.hdr_len + s.total_pay + info["pay_len"] > BUF_SIZE:
            return False
        if self.tcp and (s.raw[s.ip_hdr_len + 13] ^ info["flags"]) & ECE:
            return False
        if not s.v6 and not _ipv4_can_coalesce_id(s.raw, pkt, s.nseg):
            return False
        return self.headers_match(s.raw[:s.hdr_len], pkt[:info["hdr_len"]], s.v6, s.ip_hdr_len)

    can_append = can_append_common

    def append_payload(self, s, idx, pkt, info):  # tcp_coalesce.go:335-346, udp_coalesce.go:274-279
        s.pays.append(pkt[info["hdr_len"]:info["hdr_len"] + info["pay_len"]])
        s.members.append(idx)
        s.nseg += 1
        s.total_pay += info["pay_len"]
        s.next_seq = (info.get("seq", 0) + info["pay_len"]) & 0xFFFFFFFF
        psh = self.tcp and bool(info["flags"] & PSH)
        if psh:
            s.hdr[s.ip_hdr_len + 13] |= PSH
        return info["pay_len"] < s.gso or psh

    def flush_slot(self, s, w):  # tcp_coalesce.go:367-391, udp_coalesce.go:303-330
        total = s.hdr_len + s.total_pay
        l4 = total - s.ip_hdr_len
        hdr = s.hdr
        if s.v6:
            struct.pack_into(">H", hdr, 4, l4 & 0xFFFF)
        else:
            struct.pack_into(">H", hdr, 2, total & 0xFFFF)
            hdr[10] = hdr[11] = 0
            struct.pack_into(">H", hdr, 10, ipv4_hdr_checksum(hdr[:s.ip_hdr_len]))
        proto = TCP if self.tcp else UDP
        if not self.tcp:
            struct.pack_into(">H", hdr, s.ip_hdr_len + 4, l4 & 0xFFFF)
        if s.v6:
            ps = pseudo_sum_ipv6(hdr[8:24], hdr[24:40], proto, l4)
        else:
            ps = pseudo_sum_ipv4(hdr[12:16], hdr[16:20], proto, l4)
        struct.pack_into(">H", hdr, s.ip_hdr_len + (16 if self.tcp else 6), fold_once_no_invert(ps))
        w.WriteGSO(hdr[:s.ip_hdr_len], hdr[s.ip_hdr_len:], s.pays, self.tcp, s.first, s.members, self.lane)

    def flush(self, w):  # tcp_coalesce.go:230-254, udp_coalesce.go:179-201
        for s in self.slots:
            if s.verbatim or s.nseg == 1:
                w.Write(s.raw, s.first, self.lane)
            else:
                self.flush_slot(s, w)
        self.slots, self.open = [], {}


class TCPCoalescer(_Coalescer):
    tcp = True

    def parse_at(self, pkt, ip_hdr_len):  # tcp_coalesce.go:103-132
        r = _parse_ip_at(pkt, ip_hdr_len)
        if r is None:
            return None
        p, src, dst, v6 = r
        ip = ip_hdr_len
        if len(p) < ip + 20:
            return None
        off = (p[ip + 12] >> 4) * 4
        if off < 20 or off > 60 or len(p) < ip + off:
            return None
        sport, dport, seq = struct.unpack_from(">HHI", p, ip)
        return dict(fk=(src, dst, sport, dport, v6), v6=v6, ip_hdr_len=ip, hdr_len=ip + off,
                    pay_len=len(p) - ip - off, seq=seq, flags=p[ip + 13])

    def commit_parsed(self, idx, pkt, info):  # tcp_coalesce.go:181-228
        fl = info["flags"]
        if not fl & ACK or fl & ~(ACK | PSH | ECE) & 0xFF:
            self.seal_flow(info["fk"])
            self.add_verbatim(idx, pkt)
            return
        if info["pay_len"] == 0:  # pure ACK: seals nothing
            self.add_verbatim(idx, pkt)
            return
        self.commit_data(idx, pkt, info)

    @staticmethod
    def headers_match(a, b, v6, ip):  # tcp_coalesce.go:396-419
        if len(a) != len(b) or not _ip_headers_match(a, b, v6):
            return False
        return (a[ip:ip + 4] == b[ip:ip + 4] and a[ip + 8:ip + 13] == b[ip + 8:ip + 13]
                and a[ip + 14:ip + 16] == b[ip + 14:ip + 16] and a[ip + 18:] == b[ip + 18:])


class UDPCoalescer(_Coalescer):
    def parse_at(self, pkt, ip_hdr_len):  # udp_coalesce.go:87-112
        r = _parse_ip_at(pkt, ip_hdr_len)
        if r is None:
            return None
        p, src, dst, v6 = r
        ip = ip_hdr_len
        if len(p) < ip + 8:
            return None
        sport, dport, ulen = struct.unpack_from(">HHH", p, ip)
        if ulen < 8 or ulen > len(p) - ip:
            return None
        return dict(fk=(src, dst, sport, dport, v6), v6=v6, ip_hdr_len=ip, hdr_len=ip + 8, pay_len=ulen - 8, flags=0)

    def commit_parsed(self, idx, pkt, info):  # udp_coalesce.go:146-177
        if info["pay_len"] == 0:
            self.seal_flow(info["fk"])
            self.add_verbatim(idx, pkt)
            return
        self.commit_data(idx, pkt, info)

    @staticmethod
    def headers_match(a, b, v6, ip):  # udp_coalesce.go:334-345
        return len(a) == len(b) and _ip_headers_match(a, b, v6) and a[ip:ip + 4] == b[ip:ip + 4]


class MultiCoalescer:
    """multi_coalesce.go: Commit stages, Flush sorts by (epoch, counter), dispatches and flushes the
    lanes TCP, UDP, passthrough. tso / uso: tio.Capabilities (a lane exists only with its offload)."""

    def __init__(self, w: Writer, tso=True, uso=True):
        self.w = w
        self.tcp = TCPCoalescer(LANE_TCP) if tso else None
        self.udp = UDPCoalescer(LANE_UDP) if uso else None
        self.pt = []
        self.staged = []

    def Commit(self, idx, pkt, epoch, counter, proto, frag_any, ip_hdr_len):
        self.staged.append((epoch, counter, idx, bytes(pkt), proto, frag_any, ip_hdr_len))

    def Flush(self):
        self.staged.sort(key=lambda s: (s[0], s[1], s[2]))  # ties by input index (the reference: unspecified)
        for _, _, idx, pkt, proto, frag_any, ip in self.staged:
            if proto == TCP and self.tcp is not None:
                self.tcp.commit_staged(idx, pkt, frag_any, ip)
            elif proto == UDP and self.udp is not None:
                self.udp.commit_staged(idx, pkt, frag_any, ip)
            else:
                self.pt.append((idx, pkt))
        self.staged = []
        if self.tcp is not None:
            self.tcp.flush(self.w)
        if self.udp is not None:
            self.udp.flush(self.w)
        for idx, pkt in self.pt:
            self.w.Write(pkt, idx, LANE_PT)
        self.pt = []


def align16(x):
    return (x + 15) & ~15


def coalesce(packets, lanes=COALESCE_TCP | COALESCE_UDP, out_cap=1 << 62, max_writes=1 << 31):
    """The batch call as the model: packets = [dict(data, epoch, counter, flags=0, proto=0, ip_hdr_len=0)].
    -> (writes [dict(out_off, len, first, nseg, vnet_flags, gso_type, hdr_len, gso_size, csum_start,
    csum_offset, lane, data)], pkt_write, pkt_status)."""
    n = len(packets)
    status = [ST_OK] * n
    pw = [WRITE_NONE] * n
    w = Writer()
    m = MultiCoalescer(w, bool(lanes & COALESCE_TCP), bool(lanes & COALESCE_UDP))
    for i, p in enumerate(packets):
        fl = p.get("flags", 0)
        if fl & PLAIN_SKIP:
            status[i] = ST_SKIP
            continue
        d = p["data"]
        if fl & PLAIN_PARSED:
            if len(d) == 0:  # Offload.Write writes nothing for an empty buffer
                status[i] = ST_INVALID
                continue
            pp = (p["proto"], bool(fl & PLAIN_FRAG_ANY), p["ip_hdr_len"])
        else:
            pp = new_packet(d)
            if pp is None:  # handleOutsideMessagePacket returns before Commit (outside.go:474-479)
                status[i] = ST_INVALID
                continue
        m.Commit(i, d, p["epoch"], p["counter"], *pp)
    m.Flush()
    out, off = [], 0
    for k, wr in enumerate(w.writes):
        ln = len(wr["data"])
        if k >= max_writes or off + align16(ln) > out_cap:
            for wr2 in w.writes[k:]:
                for i in wr2["members"]:
                    status[i] = ST_NO_SPACE
            break
        for i in wr["members"]:
            pw[i] = k
        out.append(dict(wr, out_off=off, len=ln, nseg=len(wr["members"])))
        off += align16(ln)
    return out, pw, status


def plain_from_wire(pk, status, epoch, arena):
    """neb_rx_plain_from_wire's rule: pk = [(off, len, key_id)] -> [dict(off, epoch, counter, len, flags)]."""
    out = []
    for (off, ln, key), st in zip(pk, status):
        ln &= 0x7FFFFFFF
        h = arena[off:off + 16]
        if st == ST_OK and ln >= 32 and key < len(epoch) and h[0] & 0x0F == 1 and h[1] == 0:
            out.append(dict(off=off + 16, len=ln - 32, counter=int.from_bytes(h[8:16], "big"), epoch=epoch[key],
                            flags=0))
        else:
            out.append(dict(off=0, len=0, counter=0, epoch=0, flags=PLAIN_SKIP))
    return out
