"""Relay forwarding over a receive batch (neb_relay_forward_batch[_host], include/nebula_aead.h):
handleOutsideRelayPacket's ForwardingType branch (outside.go:220-240) — VerifyRelay through the
inbound tunnel's window, then SendVia (inside.go:442-501) in place under the outbound tunnel's key
and next message counters — for every packet of the batch in one call."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from .connection_state import Bits, DeviceWindows
from .inside import TX_TUNNEL_DTYPE


def relay_forward_batch(engine, alg: int, windows: Sequence[Optional[Bits]], packets: np.ndarray,
                        routes: np.ndarray, tunnels: np.ndarray, arena: np.ndarray,
                        key_hint: int = L.KEYS_MIXED) -> Tuple[np.ndarray, np.ndarray]:
    """The receive of rx_open_wire_batch over a host arena, then every verified Message/Relay packet
    with a route forwarded in place. packets: RX_PACKET_DTYPE; routes: RELAY_ROUTE_DTYPE, one per
    packet (tunnel = RELAY_NONE: do not forward); tunnels: TX_TUNNEL_DTYPE, whose message counters
    are advanced in place. Returns (status, fwd_status)."""
    n = len(packets)
    if len(routes) != n:
        raise ValueError("one route per packet")
    if tunnels.dtype != TX_TUNNEL_DTYPE or not tunnels.flags.c_contiguous:
        raise ValueError("tunnels: a contiguous TX_TUNNEL_DTYPE array (updated in place)")
    status = np.full(n, -1, dtype=np.int32)
    fwd = np.full(n, -1, dtype=np.int32)
    arr = (C.c_void_p * max(len(windows), 1))(*[(w.handle.value if w is not None else None) for w in windows])
    pk = np.ascontiguousarray(packets, dtype=L.RX_PACKET_DTYPE)
    rt = np.ascontiguousarray(routes, dtype=L.RELAY_ROUTE_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.lib().neb_relay_forward_batch_host(engine.handle, alg, arr, len(windows), vp(pk), vp(rt), n, vp(tunnels),
                                              len(tunnels), vp(arena), arena.nbytes, vp(status), vp(fwd), key_hint)
    L.check(rc, "neb_relay_forward_batch_host")
    return status, fwd


def relay_forward_batch_device(engine, alg: int, windows: DeviceWindows, d_packets, d_routes, d_tunnels, d_arena,
                               d_status, d_fwd_status, key_hint: int = L.KEYS_MIXED, stream=None) -> None:
    """relay_forward_batch with everything in device memory (torch tensors: d_packets, d_routes and
    d_tunnels uint8 of RX_PACKET_DTYPE / RELAY_ROUTE_DTYPE / TX_TUNNEL_DTYPE records, int32
    statuses). Returns once the receive is done; the forward half is enqueued on the stream
    (torch's current one by default), so the outputs are valid once it is synchronized."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
    if d_routes.numel() // L.RELAY_ROUTE_DTYPE.itemsize != n:
        raise ValueError("one route per packet")
    ntun = d_tunnels.numel() // TX_TUNNEL_DTYPE.itemsize
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_relay_forward_batch(engine.handle, alg, windows.handle, p(d_packets), p(d_routes), n,
                                         p(d_tunnels), ntun, p(d_arena), p(d_status), p(d_fwd_status), key_hint,
                                         C.c_void_p(s))
    L.check(rc, "neb_relay_forward_batch")


def rx_via_unwrap(packets: np.ndarray, via: np.ndarray, status: np.ndarray,
                  arena: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """neb_rx_via_unwrap_host: the terminal-relay unwrap rule over a finished rx_open_wire_batch, on
    the CPU. Returns (inner packets as RX_PACKET_DTYPE, inner_status: STATUS_NOT_RELAYED for the
    packets that carry no inner packet, STATUS_OK for the ones still to be received)."""
    n = len(packets)
    if len(via) != n or len(status) != n:
        raise ValueError("one via record and one status per packet")
    pk = np.ascontiguousarray(packets, dtype=L.RX_PACKET_DTYPE)
    vi = np.ascontiguousarray(via, dtype=L.RX_VIA_DTYPE)
    st = np.ascontiguousarray(status, dtype=np.int32)
    inner = np.zeros(max(n, 1), L.RX_PACKET_DTYPE)
    ist = np.full(max(n, 1), -1, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.lib().neb_rx_via_unwrap_host(vp(pk), vp(vi), vp(st), n, vp(arena), arena.nbytes, vp(inner), vp(ist))
    L.check(rc, "neb_rx_via_unwrap_host")
    return inner[:n], ist[:n]


def rx_open_via_batch(engine, alg: int, windows: Sequence[Optional[Bits]], packets: np.ndarray, via: np.ndarray,
                      arena: np.ndarray, key_hint: int = L.KEYS_MIXED,
                      inner_key_hint: int = L.KEYS_MIXED) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The receive of rx_open_wire_batch over a host arena, then every verified Message/Relay packet
    whose via record says VIA_TERMINAL unwrapped and its inner packet received the same way
    (handleOutsideRelayPacket's TerminalType branch, outside.go:210-219). via: RX_VIA_DTYPE, one per
    packet (key_id = the inner packet's tunnel). Returns (status, inner packets, inner_status)."""
    n = len(packets)
    if len(via) != n:
        raise ValueError("one via record per packet")
    status = np.full(n, -1, dtype=np.int32)
    inner = np.zeros(max(n, 1), L.RX_PACKET_DTYPE)
    ist = np.full(max(n, 1), -1, dtype=np.int32)
    arr = (C.c_void_p * max(len(windows), 1))(*[(w.handle.value if w is not None else None) for w in windows])
    pk = np.ascontiguousarray(packets, dtype=L.RX_PACKET_DTYPE)
    vi = np.ascontiguousarray(via, dtype=L.RX_VIA_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.lib().neb_rx_open_via_batch_host(engine.handle, alg, arr, len(windows), vp(pk), vp(vi), n, vp(arena),
                                            arena.nbytes, vp(status), vp(inner), vp(ist), key_hint, inner_key_hint)
    L.check(rc, "neb_rx_open_via_batch_host")
    return status, inner[:n], ist[:n]


def rx_open_via_batch_device(engine, alg: int, windows: DeviceWindows, d_packets, d_via, d_arena, d_status,
                             d_inner_packets, d_inner_status, key_hint: int = L.KEYS_MIXED,
                             inner_key_hint: int = L.KEYS_MIXED, stream=None) -> None:
    """rx_open_via_batch with everything in device memory (torch tensors: d_packets, d_inner_packets
    uint8 of RX_PACKET_DTYPE records, d_via uint8 of RX_VIA_DTYPE records, int32 statuses). Returns
    with the stream synchronized; d_inner_packets and d_inner_status go unchanged into
    plain_from_wire_device and coalesce_batch_device (nebula_amd.outside)."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
    if d_via.numel() // L.RX_VIA_DTYPE.itemsize != n or d_inner_packets.numel() // L.RX_PACKET_DTYPE.itemsize != n:
        raise ValueError("one via record and one inner record per packet")
    if d_status.numel() < n or d_inner_status.numel() < n:
        raise ValueError("one status and one inner status per packet")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_open_via_batch(engine.handle, alg, windows.handle, p(d_packets), p(d_via), n, p(d_arena),
                                       p(d_status), p(d_inner_packets), p(d_inner_status), key_hint, inner_key_hint,
                                       C.c_void_p(s))
    L.check(rc, "neb_rx_open_via_batch")


__all__ = ["relay_forward_batch", "relay_forward_batch_device", "rx_open_via_batch", "rx_open_via_batch_device",
           "rx_via_unwrap"]
