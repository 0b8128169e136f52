"""Host-side mirror of Nebula's transmit path for a batch of TUN reads, on the engine's device
TX batch (neb_tx_seal_batch[_host], and through relays neb_tx_seal_via_batch[_host];
nebula_amd/csrc/tx.hip).

Reference (slackhq/nebula):
  inside.go:154-240         sendInsideMessage: SegmentSuperpacket, one Reserve(16+len+16) slot per segment
  inside.go:178-223         its relay branch: the segment sealed at scratch[16:], then prepareSendVia
  inside.go:442-501         prepareSendVia: the relay tunnel's counter, a Message/Relay header, a second tag
  inside.go:123-146         sendInsideEncrypt: messageCounter.Add(1), header.Encode, EncryptDanger; a refused
                            segment is dropped (its counter stays used)
  overlay/tio/tio_gso_linux.go:231-280   decodeRead (virtio_net_hdr checks, FinishChecksum)
  overlay/tio/virtio/segment_linux.go    CheckValid, CorrectHdrLen, SegmentTCP, SegmentUDP, FinishChecksum
  overlay/batch/tx_batch.go:15-59        SendBatch / Arena slots handed to WriteBatch
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L

TX_PACKET_DTYPE = np.dtype({
    "names": ["in_off", "len", "tunnel", "vnet_flags", "gso_type", "hdr_len", "gso_size", "csum_start",
              "csum_offset", "reserved"],
    "formats": ["<u8", "<u4", "<u4", "u1", "u1", "<u2", "<u2", "<u2", "<u2", "<u2"],
    "offsets": [0, 8, 12, 16, 17, 18, 20, 22, 24, 26],
    "itemsize": 32,
})
TX_TUNNEL_DTYPE = np.dtype([("message_counter", "<u8"), ("key_id", "<u4"), ("remote_index", "<u4")])
TX_WIRE_DTYPE = np.dtype([("out_off", "<u8"), ("counter", "<u8"), ("len", "<u4"), ("packet", "<u4"),
                          ("segment", "<u4"), ("reserved", "<u4")])
assert TX_TUNNEL_DTYPE.itemsize == 16 and TX_WIRE_DTYPE.itemsize == 32

# virtio_net_hdr values
VNET_F_NEEDS_CSUM = 1
VNET_F_RSC_INFO = 4
GSO_NONE, GSO_TCPV4, GSO_TCPV6, GSO_UDP_L4, GSO_ECN = 0, 1, 4, 5, 0x80


def slot_bytes(seg_len: int) -> int:
    """Output bytes of one wire packet (header ‖ ct ‖ tag), 16-byte aligned."""
    return (seg_len + 32 + 15) & ~15


def slot_bytes_via(seg_len: int) -> int:
    """Output bytes of one wire packet sent through a relay (relay header ‖ header ‖ ct ‖ tag ‖ relay
    tag), 16-byte aligned."""
    return (seg_len + 64 + 15) & ~15


def _via_array(via, ntunnels: int) -> np.ndarray:
    via = np.ascontiguousarray(via, dtype=L.RELAY_ROUTE_DTYPE)
    if len(via) != ntunnels:
        raise ValueError("via needs one neb_relay_route per tunnel")
    return via


@dataclass
class TxResult:
    out: np.ndarray          # output arena
    wires: np.ndarray        # TX_WIRE_DTYPE, one per segment of the batch
    wire_status: np.ndarray  # seal status per wire (OK / EXHAUSTED)
    packet_status: np.ndarray
    tunnels: np.ndarray      # message counters advanced

    def wire_bytes(self, i: int) -> bytes:
        w = self.wires[i]
        return self.out[int(w["out_off"]):int(w["out_off"]) + int(w["len"])].tobytes()


def tx_seal_batch_host(engine, alg: int, tunnels: np.ndarray, packets: np.ndarray, in_arena: np.ndarray,
                       out_cap: int, max_wires: int, key_hint: int = L.KEYS_MIXED) -> TxResult:
    """sendInsideMessage over a whole batch of TUN reads held in host memory."""
    lib = L.lib()
    tunnels = np.ascontiguousarray(tunnels, dtype=TX_TUNNEL_DTYPE).copy()
    packets = np.ascontiguousarray(packets, dtype=TX_PACKET_DTYPE)
    in_arena = np.ascontiguousarray(in_arena, dtype=np.uint8)
    out = np.zeros(out_cap, np.uint8)
    wires = np.zeros(max_wires, TX_WIRE_DTYPE)
    wst = np.zeros(max_wires, np.int32)
    pst = np.zeros(len(packets), np.int32)
    nw = C.c_uint32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.neb_tx_seal_batch_host(engine.handle, alg, vp(tunnels), len(tunnels), vp(packets), len(packets),
                                    vp(in_arena), in_arena.nbytes, vp(out), out_cap, vp(wires), vp(wst), max_wires,
                                    C.byref(nw), vp(pst), key_hint)
    L.check(rc, "neb_tx_seal_batch_host")
    n = nw.value
    return TxResult(out, wires[:n].copy(), wst[:n].copy(), pst, tunnels)


def tx_seal_via_batch_host(engine, alg: int, tunnels: np.ndarray, via, packets: np.ndarray, in_arena: np.ndarray,
                           out_cap: int, max_wires: int, key_hint: int = L.KEYS_MIXED) -> TxResult:
    """sendInsideMessage with its relay branch over a batch of TUN reads in host memory: via[t]
    (RELAY_ROUTE_DTYPE) names the relay tunnel of tunnel t, RELAY_NONE = sent directly; via=None:
    every tunnel is direct. A via wire has TX_WIRE_VIA in wires["reserved"]."""
    lib = L.lib()
    tunnels = np.ascontiguousarray(tunnels, dtype=TX_TUNNEL_DTYPE).copy()
    via = None if via is None else _via_array(via, len(tunnels))
    packets = np.ascontiguousarray(packets, dtype=TX_PACKET_DTYPE)
    in_arena = np.ascontiguousarray(in_arena, dtype=np.uint8)
    out = np.zeros(out_cap, np.uint8)
    wires = np.zeros(max_wires, TX_WIRE_DTYPE)
    wst = np.zeros(max_wires, np.int32)
    pst = np.zeros(len(packets), np.int32)
    nw = C.c_uint32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.neb_tx_seal_via_batch_host(engine.handle, alg, vp(tunnels), len(tunnels), None if via is None else vp(via),
                                        vp(packets), len(packets), vp(in_arena), in_arena.nbytes, vp(out), out_cap,
                                        vp(wires), vp(wst), max_wires, C.byref(nw), vp(pst), key_hint)
    L.check(rc, "neb_tx_seal_via_batch_host")
    n = nw.value
    return TxResult(out, wires[:n].copy(), wst[:n].copy(), pst, tunnels)


class DeviceTxBatch:
    """A TX batch resident in device memory (torch tensors as plain allocations): the input arena
    of TUN reads, the tunnel table and the output arena; `seal()` runs neb_tx_seal_batch on torch's
    current stream; with `via` (one RELAY_ROUTE_DTYPE entry per tunnel) neb_tx_seal_via_batch."""

    def __init__(self, engine, alg: int, tunnels: np.ndarray, packets: np.ndarray, in_arena: np.ndarray,
                 out_cap: int, max_wires: int, key_hint: int = L.KEYS_MIXED, via=None):
        import torch

        dev = torch.device("cuda", engine.device)
        self.engine, self.alg, self.key_hint = engine, alg, key_hint
        self.tunnels0 = np.ascontiguousarray(tunnels, dtype=TX_TUNNEL_DTYPE).copy()
        self.tunnels = torch.from_numpy(self.tunnels0.view(np.uint8).copy()).to(dev)
        self.packets = torch.from_numpy(np.ascontiguousarray(packets, dtype=TX_PACKET_DTYPE).view(np.uint8).copy()).to(dev)
        self.npk = len(packets)
        self.ntun = len(tunnels)
        self.inp = torch.from_numpy(np.ascontiguousarray(in_arena, dtype=np.uint8).copy()).to(dev)
        self.out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)
        self.wires = torch.zeros(max_wires * TX_WIRE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.wire_status = torch.zeros(max_wires, dtype=torch.int32, device=dev)
        self.pk_status = torch.zeros(self.npk, dtype=torch.int32, device=dev)
        self.nwires = torch.zeros(1, dtype=torch.int32, device=dev)
        self.max_wires = max_wires
        self.via = None
        if via is not None:
            self.via = torch.from_numpy(_via_array(via, self.ntun).view(np.uint8).copy()).to(dev)

    def reset_counters(self) -> None:
        import torch

        self.tunnels.copy_(torch.from_numpy(self.tunnels0.view(np.uint8).copy()))

    def seal(self) -> None:
        import torch

        lib = L.lib()
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        if self.via is not None:
            rc = lib.neb_tx_seal_via_batch(self.engine.handle, self.alg, p(self.tunnels), self.ntun, p(self.via),
                                           p(self.packets), self.npk, p(self.inp), p(self.out), self.out.numel(),
                                           p(self.wires), p(self.wire_status), self.max_wires, p(self.nwires),
                                           p(self.pk_status), self.key_hint,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
            L.check(rc, "neb_tx_seal_via_batch")
            return
        rc = lib.neb_tx_seal_batch(self.engine.handle, self.alg, p(self.tunnels), self.ntun, p(self.packets),
                                   self.npk, p(self.inp), p(self.out), self.out.numel(), p(self.wires),
                                   p(self.wire_status), self.max_wires, p(self.nwires), p(self.pk_status),
                                   self.key_hint, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "neb_tx_seal_batch")

    def result(self) -> TxResult:
        n = int(self.nwires.cpu()[0])
        wires = self.wires.cpu().numpy().view(TX_WIRE_DTYPE)[:n].copy()
        return TxResult(self.out.cpu().numpy(), wires, self.wire_status.cpu().numpy()[:n].copy(),
                        self.pk_status.cpu().numpy(), self.tunnels.cpu().numpy().view(TX_TUNNEL_DTYPE).copy())


@dataclass
class SendPlan:
    """neb_tx_send_plan's six outputs (udp/udp_linux_writebatch.go:194-252: what WriteBatch packs)."""
    iov: np.ndarray          # SEND_IOV_DTYPE, niov of them
    entries: np.ndarray      # SEND_ENTRY_DTYPE, nentries of them
    wire_entry: np.ndarray   # per wire: its entry or SEND_NONE
    send_status: np.ndarray  # per wire: OK / NOT_SENT / UNROUTABLE / BAD_KEY


def send_plan_host(wires: np.ndarray, wire_status: np.ndarray, packets: np.ndarray, via, remote: np.ndarray,
                   socket_v4: bool, max_segments: int, chunk_packets: int = 128) -> SendPlan:
    """WriteBatch's packing of the sealed wires of a TX batch, held in host memory: no engine, no GPU."""
    lib = L.lib()
    wires = np.ascontiguousarray(wires, dtype=TX_WIRE_DTYPE)
    wst = np.ascontiguousarray(wire_status, dtype=np.int32)
    packets = np.ascontiguousarray(packets, dtype=TX_PACKET_DTYPE)
    remote = np.ascontiguousarray(remote, dtype=L.UDP_ADDR_DTYPE)
    via = None if via is None else _via_array(via, len(remote))
    n = len(wires)
    if len(wst) != n:
        raise ValueError("wire_status needs one entry per wire")
    iov = np.zeros(n, L.SEND_IOV_DTYPE)
    entries = np.zeros(n, L.SEND_ENTRY_DTYPE)
    went = np.zeros(n, np.uint32)
    sst = np.zeros(n, np.int32)
    ni, ne = C.c_uint32(0), C.c_uint32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.neb_tx_send_plan_host(vp(wires), vp(wst), n, vp(packets), len(packets), None if via is None else vp(via),
                                   vp(remote), len(remote), int(bool(socket_v4)), max_segments, chunk_packets, vp(iov),
                                   C.byref(ni), vp(entries), C.byref(ne), vp(went), vp(sst))
    L.check(rc, "neb_tx_send_plan_host")
    return SendPlan(iov[:ni.value].copy(), entries[:ne.value].copy(), went, sst)


class DeviceSendPlan:
    """The send plan of a DeviceTxBatch's wires, resident in device memory: `plan()` runs
    neb_tx_send_plan on torch's current stream behind the batch's seal, with no synchronisation
    between them; `result()` downloads the plan."""

    def __init__(self, batch: "DeviceTxBatch", remote: np.ndarray, socket_v4: bool, max_segments: int,
                 chunk_packets: int = 128):
        import torch

        dev = batch.wires.device
        remote = np.ascontiguousarray(remote, dtype=L.UDP_ADDR_DTYPE)
        if len(remote) != batch.ntun:
            raise ValueError("remote needs one neb_udp_addr per tunnel")
        self.batch = batch
        self.remote = torch.from_numpy(remote.view(np.uint8).copy()).to(dev)
        self.socket_v4, self.max_segments, self.chunk_packets = int(bool(socket_v4)), max_segments, chunk_packets
        n = batch.max_wires
        self.iov = torch.zeros(n * L.SEND_IOV_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.entries = torch.zeros(n * L.SEND_ENTRY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.wire_entry = torch.zeros(n, dtype=torch.int32, device=dev)
        self.send_status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=dev)  # niov, nentries

    def plan(self) -> None:
        import torch

        b = self.batch
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = L.lib().neb_tx_send_plan(b.engine.handle, p(b.wires), p(b.wire_status), p(b.nwires), b.max_wires,
                                      p(b.packets), b.npk, None if b.via is None else p(b.via), p(self.remote), b.ntun,
                                      self.socket_v4, self.max_segments, self.chunk_packets, p(self.iov),
                                      C.c_void_p(self.counts.data_ptr()), p(self.entries),
                                      C.c_void_p(self.counts.data_ptr() + 4), p(self.wire_entry), p(self.send_status),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "neb_tx_send_plan")

    def result(self) -> SendPlan:
        n = int(self.batch.nwires.cpu()[0])
        ni, ne = (int(x) for x in self.counts.cpu())
        return SendPlan(self.iov.cpu().numpy().view(L.SEND_IOV_DTYPE)[:ni].copy(),
                        self.entries.cpu().numpy().view(L.SEND_ENTRY_DTYPE)[:ne].copy(),
                        self.wire_entry.cpu().numpy().view(np.uint32)[:n].copy(), self.send_status.cpu().numpy()[:n].copy())


__all__ = ["TX_PACKET_DTYPE", "TX_TUNNEL_DTYPE", "TX_WIRE_DTYPE", "tx_seal_batch_host", "tx_seal_via_batch_host",
           "DeviceTxBatch", "TxResult", "slot_bytes", "slot_bytes_via", "SendPlan", "send_plan_host", "DeviceSendPlan"]
