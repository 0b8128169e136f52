"""firewall.Conntrack.Conns as a table (neb_conntrack_*, include/nebula_aead.h): the map that
firewall.Drop asks before it looks at any rule (firewall.go:459-478), for whole TX and RX batches,
between the resolves that emit firewall.Packet (hostmap.TxTable.resolve_*, outside.inner_*) and the
coalescer or the seal. The three operations of the reference are here: inConns (lookup), addConn (add)
and evict (firewall.go:505-630). The rules and the timer wheel stay with the caller, who gets the
packets of new flows as a work list."""
from __future__ import annotations

import ctypes as C
import ipaddress
from typing import Dict, Iterable, Optional, Tuple

import numpy as np

from . import _lib as L


def _vp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def fw_packets(rows: Iterable[Tuple[str, str, int, int, int]], fragment: bool = False) -> np.ndarray:
    """[(local address, remote address, local port, remote port, protocol)] -> FW_PACKET_DTYPE
    ("::ffff:a.b.c.d" stays a 16-byte address of family 6)."""
    rows = list(rows)
    out = np.zeros(len(rows), L.FW_PACKET_DTYPE)
    for k, (la, ra, lp, rp, proto) in enumerate(rows):
        l, r = ipaddress.ip_address(la), ipaddress.ip_address(ra)
        out[k]["family"] = l.version
        out[k]["local_addr"][:len(l.packed)] = np.frombuffer(l.packed, np.uint8)
        out[k]["remote_addr"][:len(r.packed)] = np.frombuffer(r.packed, np.uint8)
        out[k]["local_port"], out[k]["remote_port"], out[k]["protocol"] = lp, rp, proto
        out[k]["flags"] = L.FW_FRAGMENT if fragment else 0
        out[k]["gateway"] = L.GATEWAY_NONE
    return out


def key_words(fw: np.ndarray) -> np.ndarray:
    """The canonical key of each FW_PACKET_DTYPE record as the five 64-bit words a slot keeps
    (csrc/conntrack_core.hpp, ct_key_from_words): [n, 5] uint64."""
    fw = np.ascontiguousarray(fw, dtype=L.FW_PACKET_DTYPE).reshape(-1)
    q = fw.view(np.uint64).reshape(len(fw), 6)
    v4 = fw["family"] == 4
    out = np.zeros((len(fw), 5), np.uint64)
    lo = np.uint64(0xFFFFFFFF)
    out[:, 0] = np.where(v4, q[:, 0] & lo, q[:, 0])
    out[:, 1] = np.where(v4, np.uint64(0), q[:, 1])
    out[:, 2] = np.where(v4, q[:, 2] & lo, q[:, 2])
    out[:, 3] = np.where(v4, np.uint64(0), q[:, 3])
    out[:, 4] = (q[:, 4] & np.uint64(0xFFFFFFFFFFFF)) | ((fw["flags"] & L.FW_FRAGMENT).astype(np.uint64) << np.uint64(48))
    return out


def decode_slots(slots: np.ndarray) -> Dict[Tuple[int, ...], Tuple[int, int, int, int]]:
    """A dumped image -> {key words: (expires, incoming, rulesVersion, slot)} over its settled slots."""
    out = {}
    for s in np.flatnonzero((slots["state"] & np.uint64(L.CT_STATE_KIND)) == np.uint64(L.CT_STATE_SETTLED)):
        meta = int(slots["meta"][s])
        out[tuple(int(w) for w in slots["key"][s])] = (int(slots["expires"][s]), meta & 1, (meta >> 1) & 0xFFFF, int(s))
    return out


class Conntrack:
    """One neb_conntrack. engine=None: host-only (the *_host calls only); otherwise the image lives in
    the engine's device memory and only the *_device calls work."""

    def __init__(self, engine, capacity: int, seed: int = 0, tcp_ns: int = 12 * 60 * 10**9, udp_ns: int = 3 * 60 * 10**9,
                 default_ns: int = 10 * 60 * 10**9, max_batch: int = 1 << 16):
        self.engine = engine
        self.capacity, self.max_batch = capacity, max_batch
        self.handle = C.c_void_p()
        L.check(L.lib().neb_conntrack_create(engine.handle if engine is not None else None, capacity, seed, tcp_ns,
                                             udp_ns, default_ns, max_batch, C.byref(self.handle)), "neb_conntrack_create")
        self.slots = self.count()[2]

    def close(self) -> None:
        if self.handle:
            L.lib().neb_conntrack_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _e(self):
        return self.engine.handle if self.engine is not None else None

    def _stream(self, stream):
        if stream is not None:
            return stream
        if self.engine is None:
            return None
        import torch

        return torch.cuda.current_stream().cuda_stream

    def set_rules_version(self, v: int) -> None:
        L.check(L.lib().neb_conntrack_set_rules_version(self.handle, v & 0xFFFF), "neb_conntrack_set_rules_version")

    # ---- host forms -------------------------------------------------------------------------------

    def lookup_host(self, fw: np.ndarray, status: np.ndarray, now_ns: int, plain: Optional[np.ndarray] = None,
                    tx: Optional[np.ndarray] = None, work_cap: Optional[int] = None):
        """neb_conntrack_lookup_batch_host. status (int32), plain and tx are updated in place when a
        hold array is given. Returns (verdict, work[:min(nwork, work_cap)], counts)."""
        fw = np.ascontiguousarray(fw, dtype=L.FW_PACKET_DTYPE)
        n = len(fw)
        if status.dtype != np.int32 or not status.flags.c_contiguous or len(status) != n:
            raise ValueError("status: a contiguous int32 array, one per packet (updated in place)")
        cap = n if work_cap is None else work_cap
        verdict = np.zeros(n, np.uint8)
        work = np.zeros(cap, L.CT_WORK_DTYPE)
        counts = np.zeros(4, np.uint32)
        L.check(L.lib().neb_conntrack_lookup_batch_host(self.handle, _vp(fw), _vp(status), n, now_ns, _vp(verdict), _vp(plain),
                                                        _vp(tx), _vp(work) if cap else None, cap, _vp(counts)),
                "neb_conntrack_lookup_batch_host")
        return verdict, work[:min(int(counts[3]), cap)], counts

    def add_host(self, keys: np.ndarray, incoming, now_ns: int) -> np.ndarray:
        """neb_conntrack_add_batch_host -> CT_RESULT_DTYPE."""
        keys = np.ascontiguousarray(keys, dtype=L.FW_PACKET_DTYPE)
        inc = np.ascontiguousarray(incoming, dtype=np.uint8)
        if len(inc) != len(keys):
            raise ValueError("one direction per key")
        res = np.zeros(len(keys), L.CT_RESULT_DTYPE)
        L.check(L.lib().neb_conntrack_add_batch_host(self.handle, _vp(keys), _vp(inc), len(keys), now_ns, _vp(res)),
                "neb_conntrack_add_batch_host")
        return res

    def evict_host(self, keys: np.ndarray, now_ns: int, force: bool = False) -> np.ndarray:
        """neb_conntrack_evict_batch_host -> int64: -1 absent, > 0 the ns left, 0 removed."""
        keys = np.ascontiguousarray(keys, dtype=L.FW_PACKET_DTYPE)
        rem = np.zeros(len(keys), np.int64)
        L.check(L.lib().neb_conntrack_evict_batch_host(self.handle, _vp(keys), len(keys), now_ns, int(force), _vp(rem)),
                "neb_conntrack_evict_batch_host")
        return rem

    # ---- device forms: torch tensors in device memory; they only enqueue -----------------------------

    def lookup_device(self, d_fw, d_status, n: int, now_ns: int, d_verdict, d_counts, d_plain=None, d_tx=None, d_work=None,
                      work_cap: int = 0, stream=None) -> None:
        """neb_conntrack_lookup_batch: uint8 tensors of FW_PACKET_DTYPE / PLAIN_PACKET_DTYPE /
        TX_PACKET_DTYPE / CT_WORK_DTYPE records, an int32 status tensor, a uint8 verdict tensor and a
        4-element int32/uint32 counts tensor."""
        L.check(L.lib().neb_conntrack_lookup_batch(self._e(), self.handle, _dp(d_fw), _dp(d_status), n, now_ns, _dp(d_verdict),
                                                   _dp(d_plain), _dp(d_tx), _dp(d_work), work_cap, _dp(d_counts),
                                                   C.c_void_p(self._stream(stream))), "neb_conntrack_lookup_batch")

    def add_device(self, d_keys, d_incoming, n: int, now_ns: int, d_result, stream=None) -> None:
        L.check(L.lib().neb_conntrack_add_batch(self._e(), self.handle, _dp(d_keys), _dp(d_incoming), n, now_ns, _dp(d_result),
                                                C.c_void_p(self._stream(stream))), "neb_conntrack_add_batch")

    def evict_device(self, d_keys, n: int, now_ns: int, d_remaining, force: bool = False, stream=None) -> None:
        L.check(L.lib().neb_conntrack_evict_batch(self._e(), self.handle, _dp(d_keys), n, now_ns, int(force), _dp(d_remaining),
                                                  C.c_void_p(self._stream(stream))), "neb_conntrack_evict_batch")

    # ---- the table as a whole ---------------------------------------------------------------------

    def compact(self, stream=None) -> None:
        """Blocks until the table has switched to the rehashed image."""
        L.check(L.lib().neb_conntrack_compact(self.handle, C.c_void_p(self._stream(stream))), "neb_conntrack_compact")

    def count(self) -> Tuple[int, int, int]:
        """(live, tombstones, slots), after the table's enqueued work."""
        out = (C.c_uint64 * 3)()
        L.check(L.lib().neb_conntrack_count(self.handle, out), "neb_conntrack_count")
        return int(out[0]), int(out[1]), int(out[2])

    def should_compact(self) -> bool:
        live, tombs, slots = self.count()
        return 4 * (live + tombs) > 3 * slots

    def home(self, key: np.ndarray) -> int:
        """The home slot of one FW_PACKET_DTYPE record's key."""
        key = np.ascontiguousarray(key, dtype=L.FW_PACKET_DTYPE).reshape(1)
        slot = C.c_uint32()
        L.check(L.lib().neb_conntrack_home(self.handle, _vp(key), C.byref(slot)), "neb_conntrack_home")
        return slot.value

    def dump(self) -> np.ndarray:
        """The image as CT_SLOT_DTYPE, after the table's enqueued work."""
        out = np.zeros(self.slots, L.CT_SLOT_DTYPE)
        L.check(L.lib().neb_conntrack_dump(self.handle, _vp(out), self.slots), "neb_conntrack_dump")
        return out

    def entries(self):
        """{key words: (expires, incoming, rulesVersion, slot)} of the live entries."""
        return decode_slots(self.dump())


__all__ = ["Conntrack", "fw_packets", "key_words", "decode_slots"]
