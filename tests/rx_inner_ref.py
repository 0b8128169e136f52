"""TEST INFRASTRUCTURE ONLY: the model of the RX inner resolve (neb_rx_inner_batch[_host]) from
`ipaddress`, dicts and lists. Restated from slackhq/nebula, read as text:
  handleOutsideMessagePacket                outside.go:474-494
  newPacket / parseV4 / parseV6             outside.go:320-472 (incoming == true)
  IPv6FindUpperProtocol                     iputil/packet.go:349-395
  HostInfo.buildNetworks                    hostmap.go:837-857
  firewall.Drop, the two address checks     firewall.go:425-457
  NewFirewall's routableNetworks            firewall.go:154-165
It knows nothing of the hash table, of prefix-length bitmaps or of the library's parse."""
import ipaddress
import struct

OK, INVALID, NOT_MESSAGE, BAD_REMOTE, PEER_REJECTED, BAD_LOCAL = 0, 5, 7, 13, 14, 15
VPN, VPN_PEER, UNSAFE = 1, 2, 3
FRAGMENT, FRAG_ANY = 1, 2
PLAIN_PARSED, PLAIN_FRAG_ANY, PLAIN_SKIP = 1, 2, 4
GATEWAY_NONE = 0xFFFFFFFF
RX_OWN_SOURCE = 0x80000000
ICMP, TCP, UDP, ICMP6 = 1, 6, 17, 58
SKIP_RECORD = struct.pack("<QQQIHBB", 0, 0, 0, 0, 0, 0, PLAIN_SKIP)


class ParseError(Exception):
    pass


class Packet:
    """firewall.ParsedPacket, locally oriented."""

    def __init__(self):
        self.local = self.remote = None
        self.local_port = self.remote_port = self.protocol = 0
        self.fragment = self.frag_any = False
        self.ip_hdr_len = 0


def _upper6(d):
    """IPv6FindUpperProtocol -> (proto, offset, is a non-first fragment, any fragment header)"""
    nh, off, any_frag = d[6], 40, False
    for _ in range(8):
        if nh in (0, 43, 60):
            if len(d) < off + 2:
                raise ParseError("ext")
            nh, off = d[off], off + 8 * (d[off + 1] + 1)
        elif nh == 44:
            if len(d) < off + 8:
                raise ParseError("frag")
            any_frag = True
            if struct.unpack_from(">H", d, off + 2)[0] >> 3:
                return d[off], off, True, True
            nh, off = d[off], off + 8
        elif nh == 51:
            if len(d) < off + 2:
                raise ParseError("ah")
            nh, off = d[off], off + 4 * (d[off + 1] + 2)
        else:
            if off > len(d):
                raise ParseError("past")
            break
    return nh, off, False, any_frag


def new_packet_incoming(d, fp):
    """newPacket(d, true, fp); raises ParseError with fp.ip_hdr_len / fp.frag_any as left."""
    if not d:
        raise ParseError("short")
    ver = d[0] >> 4
    if ver == 4:
        if len(d) < 20:
            raise ParseError("v4 short")
        ihl = 4 * (d[0] & 15)
        if ihl < 20:
            raise ParseError("ihl")
        ff, = struct.unpack_from(">H", d, 6)
        fp.fragment, fp.frag_any, fp.ip_hdr_len, proto = bool(ff & 0x1FFF), bool(ff & 0x3FFF), ihl, d[9]
        need = ihl if fp.fragment else ihl + (6 if proto == ICMP else 4)
        if len(d) < need:
            fp.fragment = False
            raise ParseError("ports")
        fp.protocol = proto
        fp.remote, fp.local = ipaddress.IPv4Address(bytes(d[12:16])), ipaddress.IPv4Address(bytes(d[16:20]))
        if fp.fragment:
            return
        if proto == ICMP:
            fp.remote_port, = struct.unpack_from(">H", d, ihl + 4)
        else:
            fp.remote_port, fp.local_port = struct.unpack_from(">HH", d, ihl)
        return
    if ver != 6:
        raise ParseError("version")
    if len(d) < 40:
        raise ParseError("v6 short")
    proto, off, later, any_frag = _upper6(d)
    fp.frag_any, fp.ip_hdr_len = any_frag, off
    if not later:
        if proto == ICMP6:
            if len(d) < off + 4:
                raise ParseError("icmp6")
            if d[off] in (128, 129):
                if len(d) < off + 6:
                    raise ParseError("echo")
                fp.remote_port, = struct.unpack_from(">H", d, off + 4)
        elif proto in (TCP, UDP):
            if len(d) < off + 4:
                raise ParseError("ports6")
            fp.remote_port, fp.local_port = struct.unpack_from(">HH", d, off)
    fp.protocol, fp.fragment = proto, later
    fp.remote, fp.local = ipaddress.IPv6Address(bytes(d[8:24])), ipaddress.IPv6Address(bytes(d[24:40]))


def build_networks(my_networks, cert_networks, unsafe_networks=()):
    """HostInfo.buildNetworks -> {network: type}, or None in the simple case (no table)."""
    mine = [ipaddress.ip_interface(s).network for s in my_networks]
    contains = lambda ip: any(n.version == ip.version and ip in n for n in mine)  # noqa: E731
    addrs = [ipaddress.ip_interface(s).ip for s in cert_networks]
    if len(addrs) == 1 and not unsafe_networks and contains(addrs[0]):
        return None
    table = {}
    for ip in addrs:
        table[ipaddress.ip_network(ip)] = VPN if contains(ip) else VPN_PEER
    for s in unsafe_networks:
        table[ipaddress.ip_network(s, strict=False)] = UNSAFE
    return table


def lookup(table, addr):
    """bart's Lookup: the value of the longest prefix that contains addr, or None."""
    best = None
    for net, typ in table.items():
        if net.version == addr.version and addr in net and (best is None or net.prefixlen > best[0].prefixlen):
            best = (net, typ)
    return None if best is None else best[1]


def drop(fp, networks, vpn_addr0, routable):
    """The first two checks of firewall.Drop -> OK, BAD_REMOTE, PEER_REJECTED or BAD_LOCAL.
    networks: build_networks' table, or None with vpn_addr0 = h.vpnAddrs[0]."""
    if networks is None:
        if vpn_addr0 != fp.remote:
            return BAD_REMOTE
    else:
        typ = lookup(networks, fp.remote)
        if typ is None:
            return BAD_REMOTE
        if typ == VPN_PEER:
            return PEER_REJECTED
    if not any(n.version == fp.local.version and fp.local in n for n in routable):
        return BAD_LOCAL
    return OK


class Model:
    """The state the call reads: per tunnel the networks table ({network: type}; the simple case as
    its one-entry equivalent or through set_simple), and the routable set."""

    def __init__(self):
        self.tunnels = {}  # key_id -> {network: type} | ("simple", address)
        self.routable = []

    def set_routable(self, prefixes):
        self.routable = [ipaddress.ip_network(s, strict=False) for s in prefixes]

    def update(self, delete=(), put=()):
        for tunnel, prefix in delete:
            self.tunnels.get(tunnel, {}).pop(ipaddress.ip_network(prefix, strict=False), None)
        for tunnel, prefix, typ in put:
            self.tunnels.setdefault(tunnel, {})[ipaddress.ip_network(prefix, strict=False)] = typ

    def set_simple(self, tunnel, addr):
        self.tunnels[tunnel] = ("simple", ipaddress.ip_address(addr))

    def count(self):
        return sum(len(t) for t in self.tunnels.values() if isinstance(t, dict))

    def inner(self, wire, key_id, open_status, epochs, off=0, raw_len=None):
        """One packet -> (the 32 bytes of neb_plain_packet, the 48 bytes of neb_fw_packet, status).
        wire: the opened packet, header + plaintext + tag room; off: where it lies in the arena."""
        ln = (len(wire) if raw_len is None else raw_len) & ~RX_OWN_SOURCE
        if open_status != OK or ln < 32 or key_id >= len(epochs) or wire[0] & 15 != 1 or wire[1] != 0:
            return SKIP_RECORD, bytes(48), NOT_MESSAGE
        d = bytes(wire[16:ln - 16])
        fp = Packet()
        try:
            new_packet_incoming(d, fp)
        except ParseError:
            return SKIP_RECORD, struct.pack("<32sHHBBBBHHI", b"", 0, 0, 0, 0, FRAG_ANY if fp.frag_any else 0, 0, fp.ip_hdr_len,
                                            0, 0), INVALID
        t = self.tunnels.get(key_id, {})
        status = drop(fp, None, t[1], self.routable) if isinstance(t, tuple) else drop(fp, t, None, self.routable)
        flags = (FRAGMENT if fp.fragment else 0) | (FRAG_ANY if fp.frag_any else 0)
        fw = struct.pack("<16s16sHHBBBBHHI", fp.local.packed, fp.remote.packed, fp.local_port, fp.remote_port, fp.protocol,
                         fp.local.version, flags, 0, fp.ip_hdr_len, 0, GATEWAY_NONE)
        if status != OK:
            return SKIP_RECORD, fw, status
        counter, = struct.unpack_from(">Q", wire, 8)
        plain = struct.pack("<QQQIHBB", off + 16, epochs[key_id], counter, len(d), fp.ip_hdr_len, fp.protocol,
                            PLAIN_PARSED | (PLAIN_FRAG_ANY if fp.frag_any else 0))
        return plain, fw, status
