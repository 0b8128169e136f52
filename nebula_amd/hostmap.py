"""The hostmap's receive-side index lookups as a table (neb_index_table_*, neb_rx_resolve_batch[_host],
include/nebula_aead.h): what readOutsidePackets looks up per datagram before it decrypts — the
tunnel of the header's remote index (outside.go:93-106, hostmap.go:546-577), the double-encryption
check on the UDP source (outside.go:66-74) and a relay's type and target (outside.go:201-240) — for
a whole receive batch in one call, in front of rx_open_wire_batch, relay_forward_batch and
rx_open_via_batch.

And its TX-side lookups (neb_tx_table_*, neb_tx_resolve_batch[_host]): what consumeInsidePacket does
per TUN read before it can send (inside.go:19-121) — newPacket, the broadcast, self and multicast
gates, Hosts[vpnAddr], the unsafe routes' longest-prefix match and ECMP — for a whole TX batch in
one call, in front of neb_tx_seal_batch / neb_tx_seal_via_batch (TxTable).

And the state of the RX inner resolve (neb_peer_table_*; the call itself is in outside.py): every
tunnel's certificate networks as HostInfo.buildNetworks files them (hostmap.go:837-857) and the
node's routable networks (firewall.go:154-165), for the two address checks of firewall.Drop on a
whole opened batch (PeerTable, build_networks, routable)."""
from __future__ import annotations

import ctypes as C
import ipaddress
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L


def _vp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def entries(rows: Iterable[Tuple[int, int, int, int, int, int]]) -> np.ndarray:
    """[(space, index, key_id, flags, route tunnel, route remote_index)] -> INDEX_ENTRY_DTYPE"""
    rows = list(rows)
    out = np.zeros(len(rows), L.INDEX_ENTRY_DTYPE)
    for k, (space, index, key_id, flags, tunnel, remote_index) in enumerate(rows):
        out[k] = (index, space, key_id, flags, tunnel, remote_index)
    return out


def sources(addrs: Sequence[Optional[str]]) -> np.ndarray:
    """UDP source addresses (None: unknown, family 0) -> RX_SOURCE_DTYPE. "::ffff:a.b.c.d" stays a
    16-byte address, as an unmapped listener never hands it over (udp/udp_linux.go:245)."""
    out = np.zeros(len(addrs), L.RX_SOURCE_DTYPE)
    for k, a in enumerate(addrs):
        if a is None:
            continue
        ip = ipaddress.ip_address(a)
        out[k]["family"] = ip.version
        out[k]["addr"][:len(ip.packed)] = np.frombuffer(ip.packed, np.uint8)
    return out


class IndexTable:
    """One neb_index_table. engine=None: host-only (resolve_host only)."""

    def __init__(self, engine, capacity: int):
        self.engine = engine
        self.capacity = capacity
        self.handle = C.c_void_p()
        L.check(L.lib().neb_index_table_create(engine.handle if engine is not None else None, capacity,
                                               C.byref(self.handle)), "neb_index_table_create")

    def close(self) -> None:
        if self.handle:
            L.lib().neb_index_table_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def update(self, delete: Sequence[Tuple[int, int]] = (), put=(), stream=None) -> None:
        """delete: [(space, index)], applied first; put: INDEX_ENTRY_DTYPE or rows for entries().
        With an engine the device image follows on `stream` (torch's current one by default)."""
        dl = np.zeros(len(delete), L.INDEX_KEY_DTYPE)
        for k, (space, index) in enumerate(delete):
            dl[k] = (index, space)
        pt = put if isinstance(put, np.ndarray) else entries(put)
        pt = np.ascontiguousarray(pt, dtype=L.INDEX_ENTRY_DTYPE)
        L.check(L.lib().neb_index_table_update(self.handle, _vp(dl), len(dl), _vp(pt), len(pt),
                                               C.c_void_p(self._stream(stream))), "neb_index_table_update")

    def set_own_networks(self, networks: Sequence[str]) -> None:
        """networks: prefixes such as "10.1.0.0/16" or "fd00::/64" (the node's own VPN networks)."""
        nets = np.zeros(len(networks), L.CIDR_DTYPE)
        for k, s in enumerate(networks):
            n = ipaddress.ip_network(s, strict=False)
            nets[k]["family"], nets[k]["bits"] = n.version, n.prefixlen
            b = n.network_address.packed
            nets[k]["addr"][:len(b)] = np.frombuffer(b, np.uint8)
        L.check(L.lib().neb_index_table_set_own_networks(self.handle, _vp(nets), len(nets), None),
                "neb_index_table_set_own_networks")

    def count(self) -> int:
        live = C.c_uint32()
        L.check(L.lib().neb_index_table_count(self.handle, C.byref(live)), "neb_index_table_count")
        return live.value

    def probe(self, space: int, index: int) -> Tuple[bool, int, int]:
        """(found, slot, probes) from the host copy."""
        out = (C.c_uint32 * 3)()
        L.check(L.lib().neb_index_table_probe(self.handle, space, index, out), "neb_index_table_probe")
        return bool(out[0]), out[1], out[2]

    def resolve_host(self, packets: np.ndarray, arena: np.ndarray, src: Optional[np.ndarray] = None,
                     want_route: bool = True, want_via: bool = True):
        """neb_rx_resolve_batch_host. packets: RX_PACKET_DTYPE, contiguous; key_id and the
        RX_OWN_SOURCE bit of len are written in place. Returns (route or None, via or None)."""
        if packets.dtype != L.RX_PACKET_DTYPE or not packets.flags.c_contiguous:
            raise ValueError("packets: a contiguous RX_PACKET_DTYPE array (updated in place)")
        n = len(packets)
        if src is not None and len(src) != n:
            raise ValueError("one source per packet")
        src = None if src is None else np.ascontiguousarray(src, dtype=L.RX_SOURCE_DTYPE)
        route = np.zeros(n, L.RELAY_ROUTE_DTYPE) if want_route else None
        via = np.zeros(n, L.RX_VIA_DTYPE) if want_via else None
        rc = L.lib().neb_rx_resolve_batch_host(self.handle, _vp(packets), _vp(src), n, _vp(arena), arena.nbytes,
                                               _vp(route), _vp(via))
        L.check(rc, "neb_rx_resolve_batch_host")
        return route, via

    def resolve_device(self, d_packets, d_arena, d_src=None, d_route=None, d_via=None, stream=None) -> None:
        """neb_rx_resolve_batch with everything in device memory (torch uint8 tensors of
        RX_PACKET_DTYPE / RX_SOURCE_DTYPE / RELAY_ROUTE_DTYPE / RX_VIA_DTYPE records). Only enqueues:
        the outputs are valid for later work on the same stream."""
        n = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
        for t, dt in ((d_src, L.RX_SOURCE_DTYPE), (d_route, L.RELAY_ROUTE_DTYPE), (d_via, L.RX_VIA_DTYPE)):
            if t is not None and t.numel() // dt.itemsize != n:
                raise ValueError("one record per packet")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rc = L.lib().neb_rx_resolve_batch(self.engine.handle if self.engine is not None else None, self.handle,
                                          p(d_packets), p(d_src), n, p(d_arena), p(d_route), p(d_via),
                                          C.c_void_p(self._stream(stream)))
        L.check(rc, "neb_rx_resolve_batch")

    def _stream(self, stream):
        if stream is not None:
            return stream
        if self.engine is None:
            return None
        import torch

        return torch.cuda.current_stream().cuda_stream


def _addr_into(rec, a: str) -> None:
    ip = ipaddress.ip_address(a)
    rec["family"] = ip.version
    rec["addr"][:len(ip.packed)] = np.frombuffer(ip.packed, np.uint8)


def tx_addrs(addrs: Sequence[str]) -> np.ndarray:
    """VPN addresses -> TX_ADDR_DTYPE ("::ffff:a.b.c.d" stays a 16-byte address of family 6)."""
    out = np.zeros(len(addrs), L.TX_ADDR_DTYPE)
    for k, a in enumerate(addrs):
        _addr_into(out[k], a)
    return out


def tx_hosts(rows: Iterable[Tuple[str, int]]) -> np.ndarray:
    """[(VPN address, tunnel index)] -> TX_HOST_DTYPE"""
    rows = list(rows)
    out = np.zeros(len(rows), L.TX_HOST_DTYPE)
    for k, (a, tunnel) in enumerate(rows):
        _addr_into(out[k], a)
        out[k]["tunnel"] = tunnel
    return out


def tx_routes(rows: Iterable[Tuple[str, Sequence[Tuple[str, int]]]]) -> np.ndarray:
    """[(prefix, [(gateway address, weight)])] -> ROUTE_DTYPE"""
    rows = list(rows)
    out = np.zeros(len(rows), L.ROUTE_DTYPE)
    for k, (prefix, gws) in enumerate(rows):
        n = ipaddress.ip_network(prefix, strict=False)
        _addr_into(out[k], str(n.network_address))
        out[k]["bits"], out[k]["ngateways"] = n.prefixlen, len(gws)
        for j, (a, weight) in enumerate(gws[:L.ROUTE_MAX_GATEWAYS]):
            _addr_into(out[k]["gateways"][j], a)
            out[k]["gateways"][j]["weight"] = weight
    return out


def tx_own(networks: Sequence[str]) -> np.ndarray:
    """Own networks such as "10.1.0.7/16" (the node's own address with the network's length) ->
    CIDR_DTYPE, the address unmasked."""
    out = np.zeros(len(networks), L.CIDR_DTYPE)
    for k, s in enumerate(networks):
        i = ipaddress.ip_interface(s)
        _addr_into(out[k], str(i.ip))
        out[k]["bits"] = i.network.prefixlen
    return out


class TxTable:
    """One neb_tx_table: VPN address -> tunnel, the unsafe routes with their ECMP gateways, and the
    own networks of the TX gates. engine=None: host-only (resolve_host only)."""

    def __init__(self, engine, hosts: int, routes: int = 0, gateways: int = 0):
        self.engine = engine
        self.handle = C.c_void_p()
        L.check(L.lib().neb_tx_table_create(engine.handle if engine is not None else None, hosts, routes, gateways,
                                            C.byref(self.handle)), "neb_tx_table_create")

    def close(self) -> None:
        if self.handle:
            L.lib().neb_tx_table_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def update_hosts(self, delete: Sequence[str] = (), put=(), stream=None) -> None:
        """delete: addresses, applied first; put: TX_HOST_DTYPE or rows for tx_hosts(). With an
        engine the device image follows on `stream` (torch's current one by default)."""
        dl = tx_addrs(list(delete))
        pt = put if isinstance(put, np.ndarray) else tx_hosts(put)
        pt = np.ascontiguousarray(pt, dtype=L.TX_HOST_DTYPE)
        L.check(L.lib().neb_tx_table_update_hosts(self.handle, _vp(dl), len(dl), _vp(pt), len(pt),
                                                  C.c_void_p(self._stream(stream))), "neb_tx_table_update_hosts")

    def set_routes(self, routes=(), stream=None) -> None:
        """routes: ROUTE_DTYPE or rows for tx_routes(); replaces the whole set. Blocks."""
        rt = routes if isinstance(routes, np.ndarray) else tx_routes(routes)
        rt = np.ascontiguousarray(rt, dtype=L.ROUTE_DTYPE)
        L.check(L.lib().neb_tx_table_set_routes(self.handle, _vp(rt), len(rt), C.c_void_p(self._stream(stream))),
                "neb_tx_table_set_routes")

    def set_own(self, networks: Sequence[str], drop_local_broadcast: bool = False, drop_multicast: bool = False) -> None:
        nets = tx_own(networks)
        flags = (L.TX_DROP_LOCAL_BROADCAST if drop_local_broadcast else 0) | (L.TX_DROP_MULTICAST if drop_multicast else 0)
        L.check(L.lib().neb_tx_table_set_own(self.handle, _vp(nets), len(nets), flags), "neb_tx_table_set_own")

    def count(self) -> Tuple[int, int]:
        """(host entries, routes)"""
        h, r = C.c_uint32(), C.c_uint32()
        L.check(L.lib().neb_tx_table_count(self.handle, C.byref(h), C.byref(r)), "neb_tx_table_count")
        return h.value, r.value

    def probe(self, key: str, route: bool = False) -> Tuple[bool, int, int]:
        """(found, slot, probes) from the host copy; key: an address, or a prefix when route."""
        c = np.zeros(1, L.CIDR_DTYPE)
        n = ipaddress.ip_network(key, strict=False)
        _addr_into(c[0], str(n.network_address))
        c[0]["bits"] = n.prefixlen
        out = (C.c_uint32 * 3)()
        L.check(L.lib().neb_tx_table_probe(self.handle, L.TX_KIND_ROUTE if route else L.TX_KIND_HOST, _vp(c), out),
                "neb_tx_table_probe")
        return bool(out[0]), out[1], out[2]

    def resolve_host(self, packets: np.ndarray, arena: np.ndarray, arena_len: Optional[int] = None, want_fw: bool = True):
        """neb_tx_resolve_batch_host. packets: inside.TX_PACKET_DTYPE, contiguous; tunnel is written
        in place. Returns (fw or None, status), allocated per call: a caller that times the host
        form calls the C entry point on arrays of its own (tools/tx_resolve_bench.py)."""
        from .inside import TX_PACKET_DTYPE

        if packets.dtype != TX_PACKET_DTYPE or not packets.flags.c_contiguous:
            raise ValueError("packets: a contiguous TX_PACKET_DTYPE array (updated in place)")
        n = len(packets)
        fw = np.zeros(n, L.FW_PACKET_DTYPE) if want_fw else None
        status = np.zeros(n, np.int32)
        rc = L.lib().neb_tx_resolve_batch_host(self.handle, _vp(packets), n, _vp(arena),
                                               arena.nbytes if arena_len is None else arena_len, _vp(fw), _vp(status))
        L.check(rc, "neb_tx_resolve_batch_host")
        return fw, status

    def resolve_device(self, d_packets, d_in, d_fw=None, d_status=None, stream=None) -> None:
        """neb_tx_resolve_batch with everything in device memory (torch uint8 tensors of
        TX_PACKET_DTYPE / FW_PACKET_DTYPE records, an int32 tensor of statuses). Only enqueues: the
        outputs are valid for later work on the same stream."""
        n = d_packets.numel() // 32
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rc = L.lib().neb_tx_resolve_batch(self.engine.handle if self.engine is not None else None, self.handle,
                                          p(d_packets), n, p(d_in), p(d_fw), p(d_status), C.c_void_p(self._stream(stream)))
        L.check(rc, "neb_tx_resolve_batch")

    _stream = IndexTable._stream


def build_networks(my_networks: Sequence[str], cert_networks: Sequence[str],
                   unsafe_networks: Sequence[str] = ()) -> list:
    """HostInfo.buildNetworks (hostmap.go:837-857) -> [(prefix, type)] in insertion order, for
    peer_nets() / PeerTable.update: every address of the peer's certificate at full length, VPN when
    one of `my_networks` ("10.1.0.7/16": myVpnNetworksTable) contains it, else VPN_PEER; then the
    certificate's unsafe networks. The simple case, for which the reference keeps no table and
    compares with vpnAddrs[0], comes out as its equivalent: one full-length VPN entry."""
    mine = [ipaddress.ip_interface(s).network for s in my_networks]
    out = []
    for s in cert_networks:
        ip = ipaddress.ip_interface(s).ip
        inside = any(n.version == ip.version and ip in n for n in mine)
        out.append((f"{ip}/{ip.max_prefixlen}", L.NET_VPN if inside else L.NET_VPN_PEER))
    return out + [(str(ipaddress.ip_network(s, strict=False)), L.NET_UNSAFE) for s in unsafe_networks]


def routable(cert_networks: Sequence[str], unsafe_networks: Sequence[str] = ()) -> list:
    """NewFirewall's routableNetworks (firewall.go:154-165) -> prefixes for PeerTable.set_routable: the
    own certificate's addresses at full length, then its unsafe networks."""
    own = [ipaddress.ip_interface(s).ip for s in cert_networks]
    return [f"{ip}/{ip.max_prefixlen}" for ip in own] + [str(ipaddress.ip_network(s, strict=False)) for s in unsafe_networks]


def _cidr_into(rec, prefix: str) -> None:
    n = ipaddress.ip_interface(prefix)  # host bits are kept: the table masks them, as bart's Insert does
    _addr_into(rec, str(n.ip))
    rec["bits"] = n.network.prefixlen


def peer_nets(rows: Iterable[Tuple[int, str, int]]) -> np.ndarray:
    """[(tunnel, prefix, type)] -> PEER_NET_DTYPE"""
    rows = list(rows)
    out = np.zeros(len(rows), L.PEER_NET_DTYPE)
    for k, (tunnel, prefix, typ) in enumerate(rows):
        _cidr_into(out[k], prefix)
        out[k]["tunnel"], out[k]["type"] = tunnel, typ
    return out


def peer_keys(rows: Iterable[Tuple[int, str]]) -> np.ndarray:
    """[(tunnel, prefix)] -> PEER_KEY_DTYPE"""
    rows = list(rows)
    out = np.zeros(len(rows), L.PEER_KEY_DTYPE)
    for k, (tunnel, prefix) in enumerate(rows):
        _cidr_into(out[k], prefix)
        out[k]["tunnel"] = tunnel
    return out


class PeerTable:
    """One neb_peer_table: every tunnel's certificate networks (HostInfo.networks) and the node's
    routable set, for the two address checks of firewall.Drop on opened packets. engine=None:
    host-only (inner_host only)."""

    def __init__(self, engine, capacity: int):
        self.engine = engine
        self.handle = C.c_void_p()
        L.check(L.lib().neb_peer_table_create(engine.handle if engine is not None else None, capacity,
                                              C.byref(self.handle)), "neb_peer_table_create")

    def close(self) -> None:
        if self.handle:
            L.lib().neb_peer_table_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def update(self, delete=(), put=(), stream=None) -> None:
        """delete: PEER_KEY_DTYPE or rows for peer_keys(), applied first; put: PEER_NET_DTYPE or rows
        for peer_nets(). With an engine the device image follows on `stream` (torch's current one by
        default)."""
        dl = delete if isinstance(delete, np.ndarray) else peer_keys(delete)
        pt = put if isinstance(put, np.ndarray) else peer_nets(put)
        dl = np.ascontiguousarray(dl, dtype=L.PEER_KEY_DTYPE)
        pt = np.ascontiguousarray(pt, dtype=L.PEER_NET_DTYPE)
        L.check(L.lib().neb_peer_table_update(self.handle, _vp(dl), len(dl), _vp(pt), len(pt),
                                              C.c_void_p(self._stream(stream))), "neb_peer_table_update")

    def set_routable(self, prefixes: Sequence[str]) -> None:
        """prefixes: routable()'s list."""
        nets = np.zeros(len(prefixes), L.CIDR_DTYPE)
        for k, s in enumerate(prefixes):
            _cidr_into(nets[k], s)
        L.check(L.lib().neb_peer_table_set_routable(self.handle, _vp(nets), len(nets)), "neb_peer_table_set_routable")

    def count(self) -> int:
        live = C.c_uint32()
        L.check(L.lib().neb_peer_table_count(self.handle, C.byref(live)), "neb_peer_table_count")
        return live.value

    def probe(self, tunnel: int, prefix: str) -> Tuple[bool, int, int]:
        """(found, slot, probes) from the host copy."""
        key = peer_keys([(tunnel, prefix)])
        out = (C.c_uint32 * 3)()
        L.check(L.lib().neb_peer_table_probe(self.handle, _vp(key), out), "neb_peer_table_probe")
        return bool(out[0]), out[1], out[2]

    _stream = IndexTable._stream


__all__ = ["IndexTable", "entries", "sources", "TxTable", "tx_addrs", "tx_hosts", "tx_routes", "tx_own", "PeerTable",
           "build_networks", "routable", "peer_nets", "peer_keys"]
