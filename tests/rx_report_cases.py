"""Directed and random batches for the RX batch report (neb_rx_report_batch[_host]), as
rx_report_ref.Batch inputs with the toy control plane each one is replayed against.
tests/test_rx_report_cases.py asserts on the CPU that every case reaches the condition it is named
for; the host and GPU tests run them all against the model."""
from __future__ import annotations

import ipaddress
import random
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np

import rx_report_ref as M
from nebula_amd import _lib as L

FILL = 0xA5
MAX_LEN = 1400
ALL_STATUS = list(range(-1, 18))  # every status the library defines, and one it does not


def addr(ip: str, port: int) -> bytes:
    """A neb_udp_addr: 16 address bytes (family 4: the first four), port, family, reserved."""
    a = ipaddress.ip_address(ip)
    return a.packed.ljust(16, b"\0") + port.to_bytes(2, "little") + bytes([a.version, 0])


A, B, R = addr("192.0.2.1", 4242), addr("192.0.2.2", 4242), addr("198.51.100.7", 999)


def header(type_: int, sub: int, index: int, ver: int = 1, counter: int = 1) -> bytes:
    return bytes([ver << 4 | type_, sub, 0, 0]) + index.to_bytes(4, "big") + counter.to_bytes(8, "big")


class Builder:
    """Packets one after another. mode: 'entry' (from[] per receive entry with pkt_entry[], as the
    receive plan leaves them), 'packet' (from[] per packet) or 'none' (no sources)."""

    def __init__(self, mode: str = "entry", relayed: bool = False):
        self.mode, self.relayed = mode, relayed
        self.rows: List[tuple] = []
        self.hdr: List[bytes] = []
        self.frm: List[bytes] = []
        self.entry_of: Dict[bytes, int] = {}
        self.pkt_entry: List[int] = []

    def add(self, status: int, type_: int = M.MESSAGE, sub: int = 0, ver: int = 1, length: int = 64, key: int = 7,
            src: Optional[bytes] = A, own: bool = False, index: int = 0x200, entry: Optional[int] = None) -> int:
        """entry: pkt_entry[i] as given (RECV_NONE, or an index past from[]) instead of src's entry."""
        i = len(self.rows)
        self.rows.append((16 * i, length | (L.RX_OWN_SOURCE if own else 0), key, status))
        self.hdr.append(header(type_, sub, index, ver))
        src = M.NO_SOURCE if src is None else src
        if self.mode == "packet":
            self.frm.append(src)
        elif self.mode == "entry":
            if entry is None:
                if src not in self.entry_of:
                    self.entry_of[src] = len(self.frm)
                    self.frm.append(src)
                entry = self.entry_of[src]
            self.pkt_entry.append(entry)
        return i

    def batch(self) -> M.Batch:
        n = len(self.rows)
        pk = np.zeros(n, L.RX_PACKET_DTYPE)
        st = np.zeros(n, np.int32)
        for i, (off, ln, key, status) in enumerate(self.rows):
            pk[i] = (off, ln, key)
            st[i] = status
        arena = np.full(16 * n + MAX_LEN + 8, 0x5C, np.uint8)
        if n:
            arena[:16 * n] = np.frombuffer(b"".join(self.hdr), np.uint8)
        frm = None if self.mode == "none" else np.frombuffer(b"".join(self.frm), L.UDP_ADDR_DTYPE).copy()
        pe = np.array(self.pkt_entry, np.uint32) if self.mode == "entry" else None
        return M.Batch(pk, st, arena, frm, pe, self.relayed)


@dataclass
class Case:
    name: str
    batch: M.Batch
    plane: Callable[[], M.ControlPlane] = M.ControlPlane  # a fresh control plane to replay against


HEADERS = [(t, s, v) for t in range(8) for s in range(3) for v in (1, 2)] + [(15, 0, 1), (1, 255, 1), (0, 0, 0)]


def _matrix(relayed: bool, mode: str, own: bool = False) -> M.Batch:
    """Every status x every header type and subtype, valid and invalid, with and without a tunnel."""
    b = Builder(mode, relayed)
    k = 0
    for st in ALL_STATUS:
        for t, s, v in HEADERS:
            for key in (7, L.KEYS_MIXED):
                b.add(st, t, s, v, length=48 + k % 5, key=key, src=(A, B, None)[k % 3], own=own, index=0x300 + k % 3)
                k += 1
    return b.batch()


def _lens(relayed: bool) -> M.Batch:
    b = Builder("entry", relayed)
    for ln in (0, 1, 2, 15, 16, 31, 32):
        for st in ALL_STATUS:
            for t, s in ((M.MESSAGE, 0), (M.MESSAGE, 1), (M.HANDSHAKE, 0), (M.TEST, 0), (M.CONTROL, 0)):
                for key in (3, L.KEYS_MIXED):
                    b.add(st, t, s, length=ln, key=key)
    return b.batch()


def _sources(seq, key: int = 7, mode: str = "entry") -> M.Batch:
    b = Builder(mode)
    for s in seq:
        b.add(L.STATUS_OK, src=s, key=key, length=100)
    return b.batch()


def _plane(allow=lambda key, src: True, remote=None, last_roam=None, last_roam_remote=None, now=1000.0):
    def make():
        return M.ControlPlane(allow=allow, now=now, remote=dict(remote or {}), last_roam=dict(last_roam or {}),
                              last_roam_remote=dict(last_roam_remote or {}))
    return make


def _sized(n: int, seed: int) -> M.Batch:
    """n packets of a steady state: mostly opened data of a few tunnels, a little of everything else."""
    rng = random.Random(seed)
    b = Builder("entry")
    srcs = [addr(f"10.1.{k // 250}.{k % 250 + 1}", 4000 + k) for k in range(40)]
    for i in range(n):
        x = rng.random()
        key = rng.randrange(32)
        if x < 0.9:
            b.add(L.STATUS_OK, length=rng.choice((64, 1364)), key=key, src=srcs[key if rng.random() < 0.98 else key + 1])
        elif x < 0.93:
            b.add(rng.choice((L.STATUS_REPLAY, L.STATUS_AUTH_FAILED)), key=key, src=srcs[key])
        elif x < 0.95:
            b.add(L.STATUS_OK, M.MESSAGE, 1, length=200, key=40 + key % 2, src=srcs[39], index=rng.randrange(5))
        elif x < 0.97:
            b.add(L.STATUS_OK, rng.choice((M.TEST, M.LIGHTHOUSE)), 0, key=key, src=srcs[key])
        elif x < 0.98:
            b.add(L.STATUS_NOT_MESSAGE, M.HANDSHAKE, 0, key=L.KEYS_MIXED, src=srcs[38])
        elif x < 0.99:
            b.add(L.STATUS_BAD_KEY, key=L.KEYS_MIXED, src=srcs[37])
        else:
            b.add(L.STATUS_INVALID, length=rng.choice((0, 1, 5)), key=L.KEYS_MIXED, src=None, entry=L.RECV_NONE)
    return b.batch()


def directed() -> List[Case]:
    out: List[Case] = []
    add = lambda name, batch, plane=M.ControlPlane: out.append(Case(name, batch, plane))  # noqa: E731

    add("matrix", _matrix(False, "entry"))
    add("matrix_relayed", _matrix(True, "entry"))
    add("matrix_per_packet_from", _matrix(False, "packet"))
    add("matrix_no_from", _matrix(False, "none"))
    add("own_source", _matrix(False, "entry", own=True))
    add("own_source_relayed", _matrix(True, "entry", own=True))
    add("lens", _lens(False))
    add("lens_relayed", _lens(True))

    b = Builder("entry")  # padding and a hostile entry index between real packets
    b.add(L.STATUS_OK, src=A)
    b.add(L.STATUS_INVALID, length=0, key=L.KEYS_MIXED, entry=L.RECV_NONE)
    b.add(L.STATUS_OK, src=A, entry=L.RECV_NONE)  # opened, but no source: a run of its own, no roaming
    b.add(L.STATUS_OK, src=A, entry=1)  # past from[] (one entry)
    b.add(L.STATUS_OK, src=A, entry=0x7FFFFFFF)
    b.add(L.STATUS_OK, src=A)
    b.add(L.STATUS_BAD_KEY, key=L.KEYS_MIXED, entry=L.RECV_NONE)
    add("padding_and_entry_out_of_range", b.batch())

    seq = [A, A, B, A, R]
    add("roam_AABAR_allowed", _sources(seq), _plane(remote={7: R}))
    add("roam_AABAR_A_denied", _sources(seq), _plane(allow=lambda key, src: src != A, remote={7: R}))
    # the tunnel roamed from A to B a second ago: a packet from A is suppressed, then R is taken
    add("roam_back_suppressed", _sources([B, A, A, B, R, A]),
        _plane(remote={7: B}, last_roam={7: 999.5}, last_roam_remote={7: A}))
    add("roam_back_after_suppression", _sources([B, A, A, B]),
        _plane(remote={7: B}, last_roam={7: 990.0}, last_roam_remote={7: A}))
    a6, a4in6 = addr("2001:db8::1", 4242), addr("192.0.2.1", 4242)[:18] + bytes([6, 0])
    add("sources_differ_in_port", _sources([A, addr("192.0.2.1", 4243), A]))
    add("sources_differ_in_family", _sources([A, a4in6, A]))
    add("sources_differ_in_last_address_byte", _sources([a6, addr("2001:db8::2", 4242), a6, a6[:15] + b"\x03" + a6[16:]]))
    add("sources_per_packet", _sources([A, A, B, B, A], mode="packet"))

    b = Builder("entry")
    for i in range(600):
        b.add(L.STATUS_OK, key=5, src=A, length=64 + i % 7)
    add("one_tunnel_all_packets", b.batch())
    b = Builder("entry")
    for i in range(600):
        b.add(L.STATUS_OK, key=(i * 7919) % 600, src=(A, B)[i % 2])
    add("every_packet_its_own_tunnel", b.batch())
    b = Builder("entry")
    for i in range(70):
        b.add(L.STATUS_OK, key=(1, 1 | 1 << 31, 1 | 1 << 16, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, L.KEYS_MIXED)[i % 7], src=A)
    add("key_ids_differ_in_a_high_bit", b.batch())
    b = Builder("entry")
    for i in range(640):  # one relay tunnel, 64 relay indexes interleaved, some with the top bit set
        b.add(L.STATUS_OK, M.MESSAGE, 1, key=9, src=R, length=120, index=((i * 37) % 64) << 26 | (i * 37) % 64)
    add("relay_tunnel_64_interleaved_indexes", b.batch())

    for n in (1, 255, 256, 257):
        add(f"n_{n}", _sized(n, n))
    add("n_70000", _sized(70000, 70000))

    b = Builder("entry")  # sorted positions = packet indexes: heads at 255, 256, 257 and 511, 512
    for i in range(700):
        b.add(L.STATUS_OK, key=5, src=(A, B, R, A, B, R)[(i >= 255) + (i >= 256) + (i >= 257) + (i >= 511) + (i >= 512)])
    add("run_heads_at_a_block_edge", b.batch())
    b = Builder("entry")  # tunnel heads there too, and relay heads: 256 packets of index 1, then index 2
    for i in range(600):
        b.add(L.STATUS_OK, M.MESSAGE, 1, key=1 if i < 256 else 2, src=A, index=1 if i < 256 else 2)
    add("tunnel_and_relay_heads_at_a_block_edge", b.batch())
    add("empty", Builder("entry").batch())
    return out


def random_batches(seed: int, count: int, max_n: int = 3000) -> List[M.Batch]:
    rng = random.Random(seed)
    srcs = [addr(f"10.9.0.{k + 1}", 5000 + k % 3) for k in range(6)] + [addr("2001:db8::9", 5000), None]
    weights = [(L.STATUS_OK, 60), (L.STATUS_AUTH_FAILED, 4), (L.STATUS_REPLAY, 6), (L.STATUS_BAD_KEY, 6), (L.STATUS_INVALID, 8),
               (L.STATUS_NOT_MESSAGE, 8), (L.STATUS_NOT_RELAYED, 4), (L.STATUS_NO_SPACE, 2), (-1, 2)]
    statuses = [s for s, w in weights for _ in range(w)]
    out = []
    for k in range(count):
        n = min(max_n, rng.choice((rng.randrange(1, 40), rng.randrange(200, 600), rng.randrange(1, max_n + 1))))
        b = Builder(("entry", "packet", "none")[k % 3], relayed=k % 4 == 3)
        ntun, sticky = rng.choice((1, 3, 50, 2000)), rng.random()
        cur: Dict[int, bytes] = {}
        for _ in range(n):
            key = rng.choice((rng.randrange(ntun), rng.randrange(ntun) | 1 << 31, L.KEYS_MIXED, L.KEYS_MIXED - 1)) \
                if rng.random() < 0.2 else rng.randrange(ntun)
            if key not in cur or rng.random() > sticky:
                cur[key] = rng.choice(srcs)
            t, s = rng.choice(((M.MESSAGE, 0),) * 12 + ((M.MESSAGE, 1),) * 4 + tuple((t, s) for t in range(8) for s in range(2)))
            entry = rng.choice((L.RECV_NONE, 1 << 20)) if rng.random() < 0.03 else None
            b.add(rng.choice(statuses), t, s, ver=2 if rng.random() < 0.02 else 1,
                  length=rng.choice((0, 1, 2, 15, 16, 31, 32, 64, 600, 1364)) if rng.random() < 0.3 else 1364, key=key,
                  src=cur[key], own=rng.random() < 0.03, index=rng.choice((1, 2, 3, 0x80000001, rng.randrange(1 << 32))),
                  entry=entry)
        out.append(b.batch())
    return out


# ---- outputs as the tests compare them ------------------------------------------------------------

OUT_ITEMS = (("runs", L.RX_RUN_DTYPE.itemsize), ("relay_used", 8), ("work", 8))


def compare(got: Dict[str, np.ndarray], metrics: np.ndarray, counts: np.ndarray, want: M.Expected, n: int, slack: int) -> None:
    """got: the raw bytes of the three record arrays, FILL-initialised with room for n + slack records.
    Everything up to each count equals the model byte for byte; everything beyond is untouched."""
    assert counts.tolist() == want.counts.tolist(), f"counts {counts.tolist()} != {want.counts.tolist()}"
    assert metrics.tolist() == want.metrics.tolist(), f"metrics {metrics.tolist()} != {want.metrics.tolist()}"
    for (name, item), cnt, exp in zip(OUT_ITEMS, (want.counts[0], want.counts[2], want.counts[3]),
                                      (want.runs, want.relay_used, want.work)):
        raw = got[name]
        assert raw.size == (n + slack) * item
        head, tail = raw[:int(cnt) * item], raw[int(cnt) * item:]
        if head.tobytes() != exp.tobytes():
            k = next(i for i in range(int(cnt)) if head[i * item:(i + 1) * item].tobytes() != exp[i:i + 1].tobytes())
            raise AssertionError(f"{name}[{k}]: {head[k * item:(k + 1) * item].view(exp.dtype)} != {exp[k]}")
        assert (tail == FILL).all(), f"{name}: written past its count"
