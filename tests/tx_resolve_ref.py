"""TEST INFRASTRUCTURE ONLY: the model of the TX resolve (neb_tx_resolve_batch[_host]) from
`ipaddress`, dicts and lists. Restated from slackhq/nebula, read as text:
  newPacket / parseV4 / parseV6            outside.go:320-472 (incoming == false)
  IPv6FindUpperProtocol                    iputil/packet.go:349-395
  the broadcast, self, multicast gates     inside.go:43-76, pki.go:475-487
  getOrHandshakeConsiderRouting            inside.go:292-372
  RoutesFor                                overlay/tun_linux.go:366-369
  hashPacket / BalancePacket               routing/balance.go:14-39
  CalculateBucketsForGateways              routing/gateway.go:48-70
It knows nothing of the hash table."""
import copy
import ipaddress
import struct

OK, INVALID, TX_DROPPED, NO_ROUTE, NO_TUNNEL = 0, 5, 10, 11, 12
NO_TUNNEL_INDEX = GATEWAY_NONE = 0xFFFFFFFF
FRAGMENT, FRAG_ANY, GATE_BROADCAST, GATE_SELF, GATE_MULTICAST, ROUTED, ECMP_FALLBACK = 1, 2, 4, 8, 16, 32, 64
ICMP, TCP, UDP, ICMP6 = 1, 6, 17, 58


class ParseError(Exception):
    pass


class Parsed:
    def __init__(self):
        self.local = self.remote = None  # ipaddress objects; a 4-in-6 address stays an IPv6Address
        self.local_port = self.remote_port = self.protocol = 0
        self.fragment = self.frag_any = False
        self.ip_hdr_len = 0


def v6_upper(d):
    """IPv6FindUpperProtocol -> (proto, offset, is_fragment, any_fragment)"""
    if len(d) < 40:
        raise ParseError
    nh, off, any_frag = d[6], 40, False
    for _ in range(8):
        if nh in (0, 43, 60):
            if len(d) < off + 2:
                raise ParseError
            nh, off = d[off], off + ((d[off + 1] + 1) << 3)
        elif nh == 44:
            if len(d) < off + 8:
                raise ParseError
            any_frag = True
            if d[off + 2] != 0 or d[off + 3] & 0xF8:
                return d[off], off, True, True
            nh, off = d[off], off + 8
        elif nh == 51:
            if len(d) < off + 2:
                raise ParseError
            nh, off = d[off], off + ((d[off + 1] + 2) << 2)
        else:
            if off > len(d):
                raise ParseError
            break
    return nh, off, False, any_frag


def new_packet(d, fp):
    """newPacket(d, false, fp); raises ParseError with fp.ip_hdr_len / fp.frag_any as left."""
    be16 = lambda i: (d[i] << 8) | d[i + 1]  # noqa: E731
    if len(d) < 1:
        raise ParseError
    if d[0] >> 4 == 4:
        if len(d) < 20:
            raise ParseError
        ihl = (d[0] & 15) << 2
        if ihl < 20:
            raise ParseError
        ff = be16(6)
        fragment = ff & 0x1FFF != 0
        fp.frag_any = ff & 0x3FFF != 0
        fp.ip_hdr_len = ihl
        proto = d[9]
        if len(d) < ihl + (0 if fragment else 6 if proto == ICMP else 4):
            raise ParseError
        fp.fragment, fp.protocol = fragment, proto
        fp.local, fp.remote = ipaddress.IPv4Address(bytes(d[12:16])), ipaddress.IPv4Address(bytes(d[16:20]))
        if fragment:
            pass
        elif proto == ICMP:
            fp.remote_port = be16(ihl + 4)
        else:
            fp.local_port, fp.remote_port = be16(ihl), be16(ihl + 2)
        return
    if d[0] >> 4 != 6:
        raise ParseError
    proto, off, is_frag, any_frag = v6_upper(d)
    fp.frag_any, fp.ip_hdr_len = any_frag, off
    if not is_frag:
        if proto == ICMP6:
            if len(d) < off + 4:
                raise ParseError
            if d[off] in (128, 129):
                if len(d) < off + 6:
                    raise ParseError
                fp.remote_port = be16(off + 4)
        elif proto in (TCP, UDP):
            if len(d) < off + 4:
                raise ParseError
            fp.local_port, fp.remote_port = be16(off), be16(off + 2)
    fp.protocol, fp.fragment = proto, is_frag
    fp.local, fp.remote = ipaddress.IPv6Address(bytes(d[8:24])), ipaddress.IPv6Address(bytes(d[24:40]))


def is_multicast(a):
    """[ext] netip.Addr.IsMulticast: a 4-in-6 address is unmapped first."""
    if a.version == 6 and a.ipv4_mapped is not None:
        a = a.ipv4_mapped
    return a in (ipaddress.ip_network("224.0.0.0/4") if a.version == 4 else ipaddress.ip_network("ff00::/8"))


def hash_packet(local_port, remote_port):
    x = ((local_port << 16) | remote_port) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x21F0AAAD) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0xD35A2D97) & 0xFFFFFFFF
    x ^= x >> 15
    return x & 0x7FFFFFFF


def unhash_packet(h):
    """The two port pairs whose hash is h: the mixer is a bijection on 32 bits."""
    out = []
    for x in (h, h | 0x80000000):
        x ^= x >> 15
        x ^= x >> 30
        x = (x * pow(0xD35A2D97, -1, 1 << 32)) & 0xFFFFFFFF
        x ^= x >> 15
        x ^= x >> 30
        x = (x * pow(0x21F0AAAD, -1, 1 << 32)) & 0xFFFFFFFF
        x ^= x >> 16
        out.append((x >> 16, x & 0xFFFF))
    return out


def buckets(weights):
    """CalculateBucketsForGateways"""
    total, upto, out = sum(weights), 0, []
    for w in weights:
        upto += w
        out.append(((upto << 31) + total // 2) // total - 1)
    return out


def balance(h, bounds):
    for i, b in enumerate(bounds):
        if h <= b:
            return i
    raise AssertionError("buckets not calculated")


class Model:
    def __init__(self):
        self.hosts = {}  # ipaddress -> tunnel
        self.routes = []  # (network, first gateway index, [(address, bound)])
        self.own = []  # ipaddress interfaces
        self.drop_local_broadcast = self.drop_multicast = False

    def copy(self):
        return copy.deepcopy(self)

    def set_own(self, networks, drop_local_broadcast=False, drop_multicast=False):
        self.own = [ipaddress.ip_interface(s) for s in networks]
        self.drop_local_broadcast, self.drop_multicast = drop_local_broadcast, drop_multicast

    def update_hosts(self, delete=(), put=()):
        for a in delete:
            self.hosts.pop(ipaddress.ip_address(a), None)
        for a, tunnel in put:
            self.hosts[ipaddress.ip_address(a)] = tunnel

    def set_routes(self, rows):
        self.routes, first = [], 0
        for prefix, gws in rows:
            bounds = buckets([w for _, w in gws]) if len(gws) > 1 else [0x7FFFFFFF]
            self.routes.append((ipaddress.ip_network(prefix, strict=False), first,
                                [(ipaddress.ip_address(a), b) for (a, _), b in zip(gws, bounds)]))
            first += len(gws)

    def routes_for(self, a):
        best = None
        for net, first, gws in self.routes:
            if net.version == a.version and a in net and (best is None or net.prefixlen > best[0].prefixlen):
                best = (net, first, gws)
        return best

    def resolve(self, d):
        """-> (tunnel, status, the 48 bytes of neb_fw_packet)"""
        fp = Parsed()
        try:
            new_packet(d, fp)
        except ParseError:
            return NO_TUNNEL_INDEX, INVALID, struct.pack("<32sHHBBBBHHI", b"", 0, 0, 0, 0, FRAG_ANY if fp.frag_any else 0, 0,
                                                         fp.ip_hdr_len, 0, 0)
        flags = (FRAGMENT if fp.fragment else 0) | (FRAG_ANY if fp.frag_any else 0)
        tunnel, status, gateway = NO_TUNNEL_INDEX, OK, GATEWAY_NONE
        dst = fp.remote
        mine = [i for i in self.own if i.version == dst.version]
        if self.drop_local_broadcast and dst.version == 4 and any(dst == i.network.broadcast_address for i in mine):
            flags, status = flags | GATE_BROADCAST, TX_DROPPED
        elif any(dst == i.ip for i in mine):
            flags, status = flags | GATE_SELF, TX_DROPPED
        elif self.drop_multicast and is_multicast(dst):
            flags, status = flags | GATE_MULTICAST, TX_DROPPED
        elif any(dst in i.network for i in mine):
            if dst in self.hosts:
                tunnel = self.hosts[dst]
            else:
                status = NO_TUNNEL
        else:
            r = self.routes_for(dst)
            if r is None:
                status = NO_ROUTE
            else:
                _, first, gws = r
                flags |= ROUTED
                pick = balance(hash_packet(fp.local_port, fp.remote_port), [b for _, b in gws]) if len(gws) > 1 else 0
                gateway = first + pick
                chosen = gws[pick][0]
                if chosen in self.hosts:
                    tunnel = self.hosts[chosen]
                else:
                    status = NO_TUNNEL
                    for a, _ in gws if len(gws) > 1 else ():
                        if a != chosen and a in self.hosts:
                            tunnel, status, flags = self.hosts[a], OK, flags | ECMP_FALLBACK
                            break
        fw = struct.pack("<16s16sHHBBBBHHI", fp.local.packed, fp.remote.packed, fp.local_port, fp.remote_port, fp.protocol,
                         fp.local.version, flags, 0, fp.ip_hdr_len, 0, gateway)
        return tunnel, status, fw
