"""The receive side after the open (neb_rx_coalesce_batch[_host], neb_rx_plain_from_wire[_host],
include/nebula_aead.h): MultiCoalescer's Commit / Flush (overlay/batch/multi_coalesce.go:67-133) for a
whole batch — sort by (epoch, counter), coalesce in-flow TCP / UDP runs into TSO / USO superpackets,
pass the rest through, and give every TUN write its virtio_net_hdr fields.

The host form runs on the CPU (one routine's 64-packet flush); the device form keeps a batch that
neb_rx_open_wire_batch opened on the device there: receive() composes the two with
neb_rx_plain_from_wire in between.

And the receive side before the resolve (neb_rx_recv_plan[_host]): ListenOut's split of a recvmmsg
batch with UDP_GRO into wire packets (udp/udp_linux.go:237-331), recv_plan_host / recv_plan_device.

And the bookkeeping after the open (neb_rx_report_batch[_host]): readOutsidePackets' side effects
(outside.go:30-263) for a whole batch, reduced to runs per (tunnel, source), the relay indexes used,
the host's work list and the metric counts, report_host / report_device."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np

from . import _lib as L
from .connection_state import DeviceWindows, rx_open_wire_batch_device

_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def coalesce_batch_host(plain: np.ndarray, arena: np.ndarray, lanes: int = L.COALESCE_TCP | L.COALESCE_UDP,
                        out_cap: Optional[int] = None, max_writes: Optional[int] = None):
    """neb_rx_coalesce_batch_host. plain: PLAIN_PACKET_DTYPE records over `arena` (uint8, only read).
    Returns (writes[:nwrites] as TUN_WRITE_DTYPE, out arena, pkt_write, pkt_status)."""
    plain = np.ascontiguousarray(plain, dtype=L.PLAIN_PACKET_DTYPE)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    n = len(plain)
    if out_cap is None:
        out_cap = int(((plain["len"].astype(np.int64) + 15) & ~15).sum()) if n else 0
    if max_writes is None:
        max_writes = n
    out = np.zeros(max(out_cap, 1), np.uint8)
    writes = np.zeros(max(max_writes, 1), L.TUN_WRITE_DTYPE)
    nw = C.c_uint32(0)
    pw = np.full(max(n, 1), L.WRITE_NONE, np.uint32)
    ps = np.full(max(n, 1), -1, np.int32)
    rc = L.lib().neb_rx_coalesce_batch_host(_vp(plain), n, _vp(arena), arena.nbytes, _vp(out), out_cap, _vp(writes),
                                            max_writes, C.byref(nw), _vp(pw), _vp(ps), lanes)
    L.check(rc, "neb_rx_coalesce_batch_host")
    return writes[:nw.value], out, pw[:n], ps[:n]


def coalesce_batch_device(engine, d_plain, d_in, d_out, d_writes, d_nwrites, d_pkt_write, d_pkt_status,
                          lanes: int = L.COALESCE_TCP | L.COALESCE_UDP, stream=None) -> None:
    """neb_rx_coalesce_batch over torch tensors on the engine's device: d_plain uint8 of
    PLAIN_PACKET_DTYPE records, d_in / d_out uint8 arenas (out_cap = d_out.numel()), d_writes uint8 of
    TUN_WRITE_DTYPE records (max_writes = its capacity), d_nwrites one uint32 (as int32), d_pkt_write
    and d_pkt_status int32 per packet. Asynchronous on the stream (torch's current one by default)."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_plain.numel() // L.PLAIN_PACKET_DTYPE.itemsize
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_coalesce_batch(engine.handle, p(d_plain), n, p(d_in), p(d_out), d_out.numel(), p(d_writes),
                                       d_writes.numel() // L.TUN_WRITE_DTYPE.itemsize, p(d_nwrites), p(d_pkt_write),
                                       p(d_pkt_status), lanes, C.c_void_p(s))
    L.check(rc, "neb_rx_coalesce_batch")


def plain_from_wire_host(packets: np.ndarray, status: np.ndarray, epoch: np.ndarray, arena: np.ndarray) -> np.ndarray:
    """neb_rx_plain_from_wire_host: the commit records of a finished rx_open_wire_batch."""
    pk = np.ascontiguousarray(packets, dtype=L.RX_PACKET_DTYPE)
    st = np.ascontiguousarray(status, dtype=np.int32)
    ep = np.ascontiguousarray(epoch, dtype=np.uint64)
    plain = np.zeros(max(len(pk), 1), L.PLAIN_PACKET_DTYPE)
    rc = L.lib().neb_rx_plain_from_wire_host(_vp(pk), _vp(st), _vp(ep), len(ep), len(pk), _vp(arena), arena.nbytes,
                                             _vp(plain))
    L.check(rc, "neb_rx_plain_from_wire_host")
    return plain[:len(pk)]


def plain_from_wire_device(engine, d_packets, d_status, d_epoch, d_arena, d_plain, stream=None) -> None:
    """neb_rx_plain_from_wire over torch tensors (d_epoch: int64 holding the uint64 epochs)."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_plain_from_wire(engine.handle, p(d_packets), p(d_status), p(d_epoch), d_epoch.numel(), n,
                                        p(d_arena), p(d_plain), C.c_void_p(s))
    L.check(rc, "neb_rx_plain_from_wire")


def inner_host(table, packets: np.ndarray, status: np.ndarray, epoch: np.ndarray, arena: np.ndarray,
               arena_len: Optional[int] = None, want_fw: bool = True):
    """neb_rx_inner_batch_host over a hostmap.PeerTable: newPacket(incoming) and firewall.Drop's two
    address checks on a finished rx_open_wire_batch. Returns (plain, fw or None, inner status)."""
    pk = np.ascontiguousarray(packets, dtype=L.RX_PACKET_DTYPE)
    st = np.ascontiguousarray(status, dtype=np.int32)
    ep = np.ascontiguousarray(epoch, dtype=np.uint64)
    n = len(pk)
    plain = np.zeros(max(n, 1), L.PLAIN_PACKET_DTYPE)
    fw = np.zeros(max(n, 1), L.FW_PACKET_DTYPE) if want_fw else None
    inner = np.zeros(max(n, 1), np.int32)
    rc = L.lib().neb_rx_inner_batch_host(table.handle, _vp(pk), _vp(st), _vp(ep), len(ep), n, _vp(arena),
                                         arena.nbytes if arena_len is None else arena_len, _vp(plain),
                                         None if fw is None else _vp(fw), _vp(inner))
    L.check(rc, "neb_rx_inner_batch_host")
    return plain[:n], None if fw is None else fw[:n], inner[:n]


def inner_device(engine, table, d_packets, d_status, d_epoch, d_arena, d_plain, d_fw=None, d_inner_status=None,
                 stream=None) -> None:
    """neb_rx_inner_batch over torch tensors (d_epoch: int64 holding the uint64 epochs; d_fw uint8 of
    FW_PACKET_DTYPE records, d_inner_status int32, both optional). Only enqueues."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_inner_batch(engine.handle if engine is not None else None, table.handle, p(d_packets),
                                    p(d_status), p(d_epoch), d_epoch.numel(), n, p(d_arena), p(d_plain), p(d_fw),
                                    p(d_inner_status), C.c_void_p(s))
    L.check(rc, "neb_rx_inner_batch")


def recv_plan_host(entries: np.ndarray, socket_v4: bool, max_packets: int, ctrl: Optional[np.ndarray] = None,
                   ctrl_stride: int = 0):
    """neb_rx_recv_plan_host: what ListenOut does with a recvmmsg batch under UDP_GRO
    (udp/udp_linux.go:237-331). entries: RECV_ENTRY_DTYPE; ctrl: the control slots, ctrl_stride bytes
    each (None: the entries' seg_size is used). Returns (packets, sources, pkt_entry, all three over
    max_packets slots with the padding; from per entry; entry_first; npackets; nentries_done)."""
    en = np.ascontiguousarray(entries, dtype=L.RECV_ENTRY_DTYPE)
    n = len(en)
    pk = np.zeros(max(max_packets, 1), L.RX_PACKET_DTYPE)
    src = np.zeros(max(max_packets, 1), L.RX_SOURCE_DTYPE)
    pe = np.zeros(max(max_packets, 1), np.uint32)
    frm = np.zeros(max(n, 1), L.UDP_ADDR_DTYPE)
    first = np.zeros(max(n, 1), np.uint32)
    counts = np.zeros(2, np.uint32)
    if ctrl is not None:
        ctrl = np.ascontiguousarray(ctrl, dtype=np.uint8)
        if ctrl.nbytes < n * ctrl_stride:
            raise ValueError("one control slot per entry")
    rc = L.lib().neb_rx_recv_plan_host(_vp(en), n, None if ctrl is None else _vp(ctrl), ctrl_stride, int(socket_v4),
                                       _vp(pk), _vp(src), _vp(pe), max_packets, _vp(frm), _vp(first), _vp(counts))
    L.check(rc, "neb_rx_recv_plan_host")
    return pk[:max_packets], src[:max_packets], pe[:max_packets], frm[:n], first[:n], int(counts[0]), int(counts[1])


def recv_plan_device(engine, d_entries, socket_v4: bool, d_packets, d_entry_first, d_counts, d_src=None,
                     d_pkt_entry=None, d_from=None, d_ctrl=None, ctrl_stride: int = 0, stream=None) -> None:
    """neb_rx_recv_plan over torch tensors on the engine's device: d_entries uint8 of RECV_ENTRY_DTYPE
    records, d_ctrl uint8 control slots of ctrl_stride bytes (None: the entries' seg_size), d_packets
    uint8 of RX_PACKET_DTYPE records (max_packets = its capacity), d_src uint8 of RX_SOURCE_DTYPE,
    d_pkt_entry int32 per packet, d_from uint8 of UDP_ADDR_DTYPE and d_entry_first int32 per entry,
    d_counts two int32 {npackets, nentries_done}. Only enqueues: neb_rx_resolve_batch and the receive
    calls follow over all of d_packets on the same stream (torch's current one by default)."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_entries.numel() // L.RECV_ENTRY_DTYPE.itemsize
    mp = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
    if d_ctrl is not None and d_ctrl.numel() < n * ctrl_stride:
        raise ValueError("one control slot per entry")
    for t, per, cnt in ((d_src, L.RX_SOURCE_DTYPE.itemsize, mp), (d_pkt_entry, 1, mp), (d_from, L.UDP_ADDR_DTYPE.itemsize, n),
                        (d_entry_first, 1, n)):
        if t is not None and t.numel() // per < cnt:
            raise ValueError("an output is shorter than its count")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_recv_plan(engine.handle, p(d_entries) if n else None, n, p(d_ctrl), ctrl_stride, int(socket_v4),
                                  p(d_packets), p(d_src), p(d_pkt_entry), mp, p(d_from), p(d_entry_first), p(d_counts),
                                  C.c_void_p(s))
    L.check(rc, "neb_rx_recv_plan")


class Report:
    """One batch's report: runs (RX_RUN_DTYPE), relay_used (RX_RELAY_USED_DTYPE) and work (RX_WORK_DTYPE),
    each cut to its count; metrics (REPORT_NMETRICS uint64, METRIC_*); ntunnels."""

    def __init__(self, runs, relay_used, work, metrics, counts):
        c = [int(x) for x in counts]
        self.counts, self.ntunnels, self.metrics = c, c[1], metrics
        self.runs, self.relay_used, self.work = runs[:c[0]], relay_used[:c[2]], work[:c[3]]


def report_host(packets: np.ndarray, status: np.ndarray, arena: np.ndarray, frm: Optional[np.ndarray] = None,
                pkt_entry: Optional[np.ndarray] = None, relayed: bool = False, arena_len: Optional[int] = None) -> Report:
    """neb_rx_report_batch_host over a finished rx_open_wire_batch: packets (RX_PACKET_DTYPE, with the
    resolve's key_id), their statuses, the arena, and the sources: frm (UDP_ADDR_DTYPE) per receive
    entry with pkt_entry (the receive plan's outputs), per packet without it, or None."""
    pk = np.ascontiguousarray(packets, dtype=L.RX_PACKET_DTYPE)
    st = np.ascontiguousarray(status, dtype=np.int32)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    n = len(pk)
    if len(st) != n:
        raise ValueError("one status per packet")
    if frm is not None:
        frm = np.ascontiguousarray(frm, dtype=L.UDP_ADDR_DTYPE)
    if pkt_entry is not None:
        pkt_entry = np.ascontiguousarray(pkt_entry, dtype=np.uint32)
        if len(pkt_entry) != n:
            raise ValueError("one entry index per packet")
    runs = np.zeros(max(n, 1), L.RX_RUN_DTYPE)
    used = np.zeros(max(n, 1), L.RX_RELAY_USED_DTYPE)
    work = np.zeros(max(n, 1), L.RX_WORK_DTYPE)
    metrics = np.zeros(L.REPORT_NMETRICS, np.uint64)
    counts = np.zeros(4, np.uint32)
    opt = lambda a: None if a is None else _vp(a)  # noqa: E731
    rc = L.lib().neb_rx_report_batch_host(_vp(pk), _vp(st), n, _vp(arena), arena.nbytes if arena_len is None else arena_len,
                                          opt(frm), opt(pkt_entry), 0 if frm is None else len(frm),
                                          L.REPORT_RELAYED if relayed else 0, _vp(runs), _vp(used), _vp(work), _vp(metrics),
                                          _vp(counts))
    L.check(rc, "neb_rx_report_batch_host")
    return Report(runs, used, work, metrics, counts)


def report_device(engine, d_packets, d_status, d_arena, d_runs, d_relay_used, d_work, d_metrics, d_counts, d_from=None,
                  d_pkt_entry=None, relayed: bool = False, stream=None) -> None:
    """neb_rx_report_batch over torch tensors on the engine's device: d_packets uint8 of RX_PACKET_DTYPE
    records and d_status int32 as neb_rx_open_wire_batch left them, d_from uint8 of UDP_ADDR_DTYPE records
    (per receive entry with d_pkt_entry int32 per packet, else per packet), d_runs uint8 of RX_RUN_DTYPE,
    d_relay_used uint8 of RX_RELAY_USED_DTYPE and d_work uint8 of RX_WORK_DTYPE records, room for one per
    packet each, d_metrics REPORT_NMETRICS int64, d_counts four int32 {nruns, ntunnels, nrelay_used,
    nwork}. Only enqueues, behind the open on the same stream (torch's current one by default)."""
    import torch

    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n = d_packets.numel() // L.RX_PACKET_DTYPE.itemsize
    for t, per in ((d_status, 1), (d_runs, L.RX_RUN_DTYPE.itemsize), (d_relay_used, L.RX_RELAY_USED_DTYPE.itemsize),
                   (d_work, L.RX_WORK_DTYPE.itemsize), (d_pkt_entry, 1)):
        if t is not None and t.numel() // per < n:
            raise ValueError("an array is shorter than the batch")
    if d_metrics.numel() * d_metrics.element_size() < 8 * L.REPORT_NMETRICS or d_counts.numel() * d_counts.element_size() < 16:
        raise ValueError("d_metrics holds 16 uint64, d_counts four uint32")
    nfrom = 0 if d_from is None else d_from.numel() // L.UDP_ADDR_DTYPE.itemsize
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.lib().neb_rx_report_batch(engine.handle, p(d_packets), p(d_status), n, p(d_arena), p(d_from), p(d_pkt_entry), nfrom,
                                     L.REPORT_RELAYED if relayed else 0, p(d_runs), p(d_relay_used), p(d_work), p(d_metrics),
                                     p(d_counts), C.c_void_p(s))
    L.check(rc, "neb_rx_report_batch")


class TunWrite:
    """One write to the TUN: the virtio_net_hdr fields and the bytes."""

    def __init__(self, rec, data: bytes):
        self.flags, self.gso_type = int(rec["vnet_flags"]), int(rec["gso_type"])
        self.hdr_len, self.gso_size = int(rec["hdr_len"]), int(rec["gso_size"])
        self.csum_start, self.csum_offset = int(rec["csum_start"]), int(rec["csum_offset"])
        self.first, self.nseg, self.lane = int(rec["first"]), int(rec["nseg"]), int(rec["lane"])
        self.data = data


class MultiCoalescer:
    """batch.MultiCoalescer's surface: Commit stages a plaintext packet with its sort key and the
    firewall's parse (None: derived as newPacket does), Flush returns the TUN writes in the
    reference's order. engine=None runs the host form; with an engine the batch goes through the
    device form."""

    def __init__(self, tso: bool = True, uso: bool = True, engine=None):
        self.lanes = (L.COALESCE_TCP if tso else 0) | (L.COALESCE_UDP if uso else 0)
        self.engine = engine
        self._pk: List[Tuple[bytes, int, int, Optional[Tuple[int, bool, int]]]] = []

    def Commit(self, pkt: bytes, epoch: int, counter: int, pp: Optional[Tuple[int, bool, int]] = None) -> None:
        """pp: (Protocol, FragAny, IPHdrLen) of firewall.ParsedPacket."""
        self._pk.append((bytes(pkt), epoch, counter, pp))

    def _stage(self):
        plain = np.zeros(len(self._pk), L.PLAIN_PACKET_DTYPE)
        parts, off = [], 0
        for i, (d, ep, ctr, pp) in enumerate(self._pk):
            plain[i] = (off, ep, ctr, len(d), pp[2] if pp else 0, pp[0] if pp else 0,
                        (L.PLAIN_PARSED | (L.PLAIN_FRAG_ANY if pp[1] else 0)) if pp else 0)
            parts.append(d)
            off += len(d)
        return plain, np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy()

    def Flush(self) -> List[TunWrite]:
        if not self._pk:
            return []
        plain, arena = self._stage()
        self._pk = []
        if self.engine is None:
            writes, out, _, _ = coalesce_batch_host(plain, arena, self.lanes)
        else:
            import torch

            dev = torch.device("cuda", self.engine.device)
            n = len(plain)
            cap = int(((plain["len"].astype(np.int64) + 15) & ~15).sum()) + 16
            t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
            d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
            d_writes = torch.zeros(n * L.TUN_WRITE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_nw = torch.zeros(1, dtype=torch.int32, device=dev)
            d_pw = torch.zeros(n, dtype=torch.int32, device=dev)
            d_ps = torch.zeros(n, dtype=torch.int32, device=dev)
            d_plain, d_in = t(plain), t(arena)
            coalesce_batch_device(self.engine, d_plain, d_in, d_out, d_writes, d_nw, d_pw, d_ps, self.lanes)
            torch.cuda.synchronize(dev)
            writes = d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:int(d_nw.item())]
            out = d_out.cpu().numpy()
        return [TunWrite(w, out[int(w["out_off"]):int(w["out_off"]) + int(w["len"])].tobytes()) for w in writes]


def receive(engine, alg: int, windows: DeviceWindows, d_packets, d_arena, d_status, d_epoch, d_plain, d_out,
            d_writes, d_nwrites, d_pkt_write, d_pkt_status, lanes: int = L.COALESCE_TCP | L.COALESCE_UDP,
            key_hint: int = L.KEYS_MIXED, stream=None, peers=None, d_fw=None, d_inner_status=None) -> None:
    """Wire packets to TUN writes on the device: neb_rx_open_wire_batch (the gate, the replay windows,
    Decrypt / VerifyRelay) -> neb_rx_plain_from_wire (opened data messages become commit records,
    epoch = d_epoch[key_id]) -> neb_rx_coalesce_batch. The caller marks firewall drops by or-ing
    PLAIN_SKIP into d_plain's flags between the last two steps if it filters; this composition commits
    every opened data message. With `peers` (a hostmap.PeerTable on the engine) neb_rx_inner_batch
    takes the middle step's place: a packet whose inner source is not the peer's, or whose inner
    destination is not ours, is not committed, and d_fw / d_inner_status (optional) say why. The
    outputs are valid once the stream is synchronized."""
    rx_open_wire_batch_device(engine, alg, windows, d_packets, d_arena, d_status, key_hint, stream)
    if peers is None:
        plain_from_wire_device(engine, d_packets, d_status, d_epoch, d_arena, d_plain, stream)
    else:
        inner_device(engine, peers, d_packets, d_status, d_epoch, d_arena, d_plain, d_fw, d_inner_status, stream)
    coalesce_batch_device(engine, d_plain, d_arena, d_out, d_writes, d_nwrites, d_pkt_write, d_pkt_status, lanes,
                          stream)


__all__ = ["MultiCoalescer", "TunWrite", "coalesce_batch_host", "coalesce_batch_device", "plain_from_wire_host",
           "plain_from_wire_device", "inner_host", "inner_device", "receive", "recv_plan_host", "recv_plan_device", "Report", "report_host", "report_device"]
