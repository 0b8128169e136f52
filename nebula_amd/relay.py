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


__all__ = ["relay_forward_batch", "relay_forward_batch_device"]
