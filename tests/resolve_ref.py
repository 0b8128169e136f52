"""TEST INFRASTRUCTURE ONLY: the lookups readOutsidePackets makes per datagram before it decrypts,
as plain dicts, for tests/test_resolve_host.py and tests/test_gpu_resolve.py. Written from
outside.go; shares nothing with nebula_amd/csrc/index_core.hpp.

  outside.go:66-74    not relayed and myVpnNetworksTable.Contains(source): the datagram is refused
  outside.go:93-100   Message/Relay: hostMap.QueryRelayIndex(h.RemoteIndex), else QueryIndexCached
  outside.go:201-240  handleOutsideRelayPacket: the relay's type; TerminalType: the inner packet is
                      ours (readOutsidePackets again on packet[16:len-16]); ForwardingType: the
                      target host and its relay index

hostMap.Indexes and hostMap.Relays are two maps from a local index (hostmap.go:60-61); here one
dict keyed by (space, index). netip.Prefix.Contains is ipaddress's `in`: an IPv4 address is in no
IPv6 network, and ::ffff:a.b.c.d is an IPv6 address."""
import ipaddress

TUNNEL, RELAY = 0, 1
MIXED = 0xFFFFFFFF  # no tunnel
RELAY_NONE = 0xFFFFFFFF
VIA_TERMINAL = 1
OWN_SOURCE = 0x80000000


class Model:
    def __init__(self):
        self.entries = {}  # (space, index) -> (key_id, flags, route tunnel, route remote_index)
        self.networks = []

    def update(self, delete=(), put=()):
        """delete: [(space, index)]; put: [(space, index, key_id, flags, tunnel, remote_index)]"""
        for k in delete:
            self.entries.pop(tuple(k), None)
        for space, index, key_id, flags, tunnel, remote_index in put:
            self.entries[(space, index)] = (key_id, flags, tunnel, remote_index)

    def copy(self):
        m = Model()
        m.entries = dict(self.entries)
        m.networks = list(self.networks)
        return m

    def set_own_networks(self, networks):
        self.networks = [ipaddress.ip_network(n, strict=False) for n in networks]

    def own_source(self, src):
        if src is None:
            return False
        ip = ipaddress.ip_address(src)
        return any(ip.version == n.version and ip in n for n in self.networks)

    def _entry(self, header):
        """The entry a 16-byte header names: Message with subtype MessageRelay asks the relay map."""
        relay = header[0] & 15 == 1 and header[1] == 1
        index = int.from_bytes(header[4:8], "big")
        return relay, self.entries.get((RELAY if relay else TUNNEL, index))

    def resolve_one(self, packet, src=None):
        """packet: the datagram's bytes. Returns (key_id, own source, (route), (via))."""
        key, route, via = MIXED, (RELAY_NONE, 0), [MIXED, 0]
        own = self.own_source(src)
        if len(packet) >= 16:
            relay, e = self._entry(packet[:16])
            if e is not None:
                key = e[0]
                if relay:
                    if e[2] != RELAY_NONE:
                        route = (e[2], e[3])
                    if e[1] & VIA_TERMINAL:
                        via[1] = VIA_TERMINAL
                        if len(packet) >= 48:  # an inner header inside header || inner || tag
                            _, inner = self._entry(packet[16:32])
                            if inner is not None:
                                via[0] = inner[0]
        return key, own, route, tuple(via)

    def resolve(self, arena, packets, srcs=None):
        """arena: bytes-like; packets: [(off, len with or without OWN_SOURCE)].
        Returns ([key_id], [len with the bit], [route], [via])."""
        keys, lens, routes, vias = [], [], [], []
        for i, (off, ln) in enumerate(packets):
            n = ln & ~OWN_SOURCE
            k, own, r, v = self.resolve_one(bytes(arena[off:off + n]), None if srcs is None else srcs[i])
            keys.append(k)
            lens.append(ln | (OWN_SOURCE if own else 0))
            routes.append(r)
            vias.append(v)
        return keys, lens, routes, vias
