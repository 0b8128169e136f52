"""A per-packet model of what a received batch does to the control plane, for the RX batch report
(neb_rx_report_batch, include/nebula_aead.h).

walk() goes through a batch packet by packet in the order of readOutsidePackets (outside.go:30-189)
and handleOutsideRelayPacket (:191-200), against a toy control plane (ControlPlane): messageMetrics,
connectionManager.In / RelayUsed, handleHostRoaming (:279-309) with an allow list and a frozen clock,
and a log of what the reference dispatches. Where the reference decides by looking a tunnel up,
decrypting or checking the replay window, the walk takes the batch's finished status instead: that is
what neb_rx_open_wire_batch left behind.

report() states the report itself (runs, relay_used, work, metrics, counts) and replay() applies a
report to a ControlPlane the way INTEGRATION.md §3 tells a caller to: In once per tunnel,
handleHostRoaming once per run, RelayUsed per index, the work list in order."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from nebula_amd import _lib as L

NO_SOURCE = bytes(20)
ROAMING_SUPPRESS_SECONDS = 2  # RoamingSuppressSeconds (hostmap.go:35)

# header types (header/header.go)
HANDSHAKE, MESSAGE, RECV_ERROR, LIGHTHOUSE, TEST, CLOSE_TUNNEL, CONTROL = range(7)


def valid_subtype(t: int, s: int) -> bool:
    """IsValidSubType (header.go:192-205)."""
    if t in (MESSAGE, TEST):
        return s <= 1
    return t in (HANDSHAKE, RECV_ERROR, LIGHTHOUSE, CLOSE_TUNNEL, CONTROL) and s == 0


def rx_slot(t: int, s: int) -> int:
    """The row of newMessageMetrics (message_metrics.go:52-77) Rx(t, s) counts in; a type without a
    row (Control) goes to rx.other."""
    rows = {HANDSHAKE: [L.METRIC_RX_HANDSHAKE], RECV_ERROR: [L.METRIC_RX_RECV_ERROR], LIGHTHOUSE: [L.METRIC_RX_LIGHTHOUSE],
            TEST: [L.METRIC_RX_TEST_REQUEST, L.METRIC_RX_TEST_RESPONSE], CLOSE_TUNNEL: [L.METRIC_RX_CLOSE_TUNNEL]}
    row = rows.get(t, [])
    return row[s] if s < len(row) else L.METRIC_RX_OTHER


@dataclass
class Batch:
    """A finished receive batch as the report's inputs."""
    pk: np.ndarray  # RX_PACKET_DTYPE
    status: np.ndarray  # int32
    arena: np.ndarray  # uint8
    frm: Optional[np.ndarray] = None  # UDP_ADDR_DTYPE
    pkt_entry: Optional[np.ndarray] = None  # uint32
    relayed: bool = False

    def __len__(self) -> int:
        return len(self.pk)

    def source(self, i: int) -> bytes:
        """The 20 bytes of packet i's source, NO_SOURCE when it has none."""
        if self.frm is None or self.relayed:
            return NO_SOURCE
        j = int(self.pkt_entry[i]) if self.pkt_entry is not None else i
        if j == L.RECV_NONE or j >= len(self.frm):
            return NO_SOURCE
        return self.frm[j].tobytes()


@dataclass
class Packet:
    """What the walk sees of one packet."""
    i: int
    status: int
    len: int
    own: bool
    key_id: int
    has_header: bool
    ver: int = 0
    type: int = 0
    sub: int = 0
    index: int = 0


def packet(b: Batch, i: int) -> Packet:
    raw, off = int(b.pk["len"][i]), int(b.pk["off"][i])
    ln = raw & ~L.RX_OWN_SOURCE
    p = Packet(i, int(b.status[i]), ln, bool(raw & L.RX_OWN_SOURCE), int(b.pk["key_id"][i]), ln >= 16)
    if p.has_header:
        h = b.arena[off:off + 16]
        p.ver, p.type, p.sub = int(h[0]) >> 4, int(h[0]) & 15, int(h[1])
        p.index = int.from_bytes(h[4:8].tobytes(), "big")
    return p


@dataclass
class ControlPlane:
    """The state a received batch changes. remote / last_roam / last_roam_remote are per tunnel
    (hostinfo.remote, lastRoam, lastRoamRemote); allow(key_id, source) is the lighthouse's remote allow
    list; now is frozen."""
    allow: Callable[[int, bytes], bool] = lambda key, src: True
    now: float = 1000.0
    remote: Dict[int, bytes] = field(default_factory=dict)
    last_roam: Dict[int, float] = field(default_factory=dict)
    last_roam_remote: Dict[int, bytes] = field(default_factory=dict)
    in_flags: set = field(default_factory=set)
    relay_used: set = field(default_factory=set)
    metrics: List[int] = field(default_factory=lambda: [0] * L.REPORT_NMETRICS)
    log: List[Tuple[int, int]] = field(default_factory=list)  # (WORK_*, packet)
    roams: int = 0  # how often a remote changed
    denied: int = 0
    suppressed: int = 0

    def handle_host_roaming(self, key: int, via: bytes) -> None:
        """outside.go:279-309, for a packet that is not relayed."""
        cur = self.remote.get(key, NO_SOURCE)
        if cur == via:
            return
        if not self.allow(key, via):
            self.denied += 1
            return
        if key in self.last_roam and via == self.last_roam_remote.get(key) and \
                self.now - self.last_roam[key] < ROAMING_SUPPRESS_SECONDS:
            self.suppressed += 1
            return
        self.last_roam[key] = self.now
        self.last_roam_remote[key] = cur
        self.remote[key] = via
        self.roams += 1

    def state(self):
        """Everything but the counters of how the state was reached."""
        return (dict(self.remote), dict(self.last_roam), dict(self.last_roam_remote), set(self.in_flags),
                set(self.relay_used), list(self.metrics), list(self.log))


def walk(b: Batch, cp: ControlPlane) -> None:
    """The batch packet by packet."""
    m = cp.metrics
    for i in range(len(b)):
        p = packet(b, i)
        # h.Parse, version, IsValidSubType, the double-encryption check: each RxInvalid (outside.go:32-74).
        # The gate refuses a short tunnel packet with the same status (:111-117).
        if p.status == L.STATUS_INVALID and p.len > 1:
            m[L.METRIC_RX_INVALID] += 1
        past_gates = p.has_header and p.ver == 1 and valid_subtype(p.type, p.sub) and (b.relayed or not p.own)
        if past_gates and p.type != MESSAGE:  # :77-79
            m[rx_slot(p.type, p.sub)] += 1
        relay = p.has_header and p.type == MESSAGE and p.sub == 1
        if p.status == L.STATUS_NOT_MESSAGE and p.has_header:  # :82-90, and one more level of relay
            if p.type == HANDSHAKE:
                cp.log.append((L.WORK_HANDSHAKE, i))
            elif p.type == RECV_ERROR:
                cp.log.append((L.WORK_RECV_ERROR, i))
            elif b.relayed and relay:
                cp.log.append((L.WORK_NESTED_RELAY, i))
        elif p.status == L.STATUS_BAD_KEY and p.key_id == L.KEYS_MIXED:  # :104-109
            m[L.METRIC_NO_TUNNEL] += 1
            if not b.relayed and p.has_header:
                cp.log.append((L.WORK_SEND_RECV_ERROR, i))
        elif p.status == L.STATUS_AUTH_FAILED:  # :123-128, :134-139
            m[L.METRIC_AUTH_FAILED] += 1
        elif p.status == L.STATUS_REPLAY:
            m[L.METRIC_REPLAY] += 1
        elif p.status == L.STATUS_OK:
            m[L.METRIC_OPENED] += 1
            m[L.METRIC_OPENED_BYTES] += p.len
            via = b.source(i)
            if via[18] != 0:  # family; :142 / :196; a relayed packet never roams (:281)
                cp.handle_host_roaming(p.key_id, via)
            cp.in_flags.add(p.key_id)  # :143 / :198
            if relay:
                cp.relay_used.add(p.index)  # :199
            elif p.has_header:
                kind = {LIGHTHOUSE: L.WORK_LIGHTHOUSE, CLOSE_TUNNEL: L.WORK_CLOSE_TUNNEL, CONTROL: L.WORK_CONTROL}.get(p.type)
                if p.type == TEST and p.sub == 0:
                    kind = L.WORK_TEST_REQUEST
                if kind:
                    cp.log.append((kind, i))


@dataclass
class Expected:
    runs: np.ndarray
    relay_used: np.ndarray
    work: np.ndarray
    metrics: np.ndarray
    counts: np.ndarray  # {nruns, ntunnels, nrelay_used, nwork}


def report(b: Batch) -> Expected:
    """The report of include/nebula_aead.h, stated directly."""
    cp = ControlPlane()
    walk(b, cp)  # for the metrics and the dispatch log, which need no state
    auth = [(int(b.pk["key_id"][i]), i) for i in range(len(b)) if int(b.status[i]) == L.STATUS_OK]
    auth.sort()
    runs: List[list] = []  # [bytes, key, first, packets, source]
    for key, i in auth:
        src, ln = b.source(i), int(b.pk["len"][i]) & ~L.RX_OWN_SOURCE
        if runs and runs[-1][1] == key and runs[-1][4] == src:
            runs[-1][0] += ln
            runs[-1][3] += 1
        else:
            runs.append([ln, key, i, 1, src])
    used: Dict[int, int] = {}
    for _, i in auth:
        p = packet(b, i)
        if p.has_header and p.type == MESSAGE and p.sub == 1:
            used[p.index] = used.get(p.index, 0) + 1
    out_runs = np.zeros(len(runs), L.RX_RUN_DTYPE)
    for r, (nbytes, key, first, cnt, src) in enumerate(runs):
        out_runs[r] = (nbytes, key, first, cnt, np.frombuffer(src, L.UDP_ADDR_DTYPE)[0])
    out_used = np.array(sorted(used.items()), dtype=np.uint32).reshape(-1, 2).copy().view(L.RX_RELAY_USED_DTYPE).reshape(-1)
    out_work = np.array([(i, k) for k, i in cp.log], dtype=np.uint32).reshape(-1, 2).copy().view(L.RX_WORK_DTYPE).reshape(-1)
    counts = np.array([len(runs), len({k for k, _ in auth}), len(used), len(cp.log)], np.uint32)
    return Expected(out_runs, out_used, out_work, np.array(cp.metrics, np.uint64), counts)


def replay(runs: np.ndarray, relay_used: np.ndarray, work: np.ndarray, metrics: np.ndarray, cp: ControlPlane) -> None:
    """What a caller does with a report: a loop over runs, not over packets."""
    for k in range(L.REPORT_NMETRICS):
        cp.metrics[k] += int(metrics[k])
    for r in runs:
        key = int(r["key_id"])
        cp.in_flags.add(key)  # once per distinct key_id is enough; the set makes a repeat harmless
        if int(r["from"]["family"]) != 0:
            cp.handle_host_roaming(key, r["from"].tobytes())
    for u in relay_used:
        cp.relay_used.add(int(u["index"]))
    for w in work:
        cp.log.append((int(w["kind"]), int(w["packet"])))
