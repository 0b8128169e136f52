"""Models of the TX send plan (neb_tx_send_plan[_host]), in plain Python over plain lists.

sequential(b)  batchWriter.WriteBatch's packing loop with planRun (udp/udp_linux_writebatch.go:194-252,
               :312-346), restated from their semantics, with the wire -> destination step in front:
               a chunk loop, an entry loop with an iovec budget, runs planned one after another, the
               runs of destinations the socket cannot address skipped without using budget.
parallel(b)    the decomposition the device form uses, written from its statement alone (hard
               boundaries, plateaus, one carried bit per plateau as a function {0,1} -> {0,1}, all
               bits from one scan under composition), independently of csrc/send_core.hpp.

Both return Plan(iov, entries, wire_entry, send_status):
  iov      [(off, len, wire)]
  entries  [(iov_first, niov, seg_size, dst, bytes)]
"""
from __future__ import annotations

from dataclasses import dataclass, field

OK, BAD_KEY, UNROUTABLE, NOT_SENT = 0, 3, 16, 17
NONE = 0xFFFFFFFF
MAX_BYTES = 65000
WIRE_VIA = 1


@dataclass
class Batch:
    lens: list            # per wire: len
    packet: list          # per wire: index of its packet
    flags: list           # per wire: neb_tx_wire.reserved
    status: list          # per wire: wire_status
    pkt_tunnel: list      # per packet: tunnel
    remote: list          # per tunnel: (family, addr: bytes(16), port, reserved)
    via: list | None = None   # per tunnel: relay tunnel (NONE: direct)
    socket_v4: bool = True
    max_segments: int = 63
    chunk_packets: int = 128
    out_off: list = field(default_factory=list)  # per wire; default: 16-aligned slots in wire order

    def __post_init__(self):
        if not self.out_off:
            off = 0
            for ln in self.lens:
                self.out_off.append(off)
                off += (ln + 15) & ~15


@dataclass
class Plan:
    iov: list
    entries: list
    wire_entry: list
    send_status: list


def routable(addr, socket_v4: bool) -> bool:
    family, a = addr[0], addr[1]
    if family == 4:
        return True
    if family != 6:
        return False
    return (not socket_v4) or a[:12] == b"\0" * 10 + b"\xff\xff"


def resolve(b: Batch):
    """Per wire: (send_status, dst tunnel, destination key). The key of a bad index is the wire's own."""
    out = []
    nt = len(b.remote)
    for i in range(len(b.lens)):
        if b.status[i] != OK:
            out.append((NOT_SENT, NONE, None))
            continue
        bad = (BAD_KEY, NONE, ("bad", i))
        if b.packet[i] >= len(b.pkt_tunnel):
            out.append(bad)
            continue
        t = b.pkt_tunnel[b.packet[i]]
        if t >= nt:
            out.append(bad)
            continue
        if b.flags[i] & WIRE_VIA:
            if b.via is None or b.via[t] >= nt:
                out.append(bad)
                continue
            t = b.via[t]
        addr = tuple(b.remote[t])
        out.append((OK if routable(addr, b.socket_v4) else UNROUTABLE, t, addr))
    return out


# ---- the sequential model ----------------------------------------------------------------------------

def _plan_run(bufs, addrs, start, budget, gso, max_segments):
    if start >= len(bufs) or budget < 1:
        return 0, 0
    seg = bufs[start]
    if not gso or seg == 0 or seg > MAX_BYTES:
        return 1, seg
    max_len = min(max_segments, budget)
    run, total = 1, seg
    while run < max_len and start + run < len(bufs):
        nxt = bufs[start + run]
        if nxt == 0 or nxt > seg:
            break
        if addrs[start + run] != addrs[start]:
            break
        if total + nxt > MAX_BYTES:
            break
        total += nxt
        run += 1
        if nxt < seg:
            break
    return run, seg


def sequential(b: Batch) -> Plan:
    res = resolve(b)
    n = len(b.lens)
    sent = [i for i in range(n) if res[i][0] != NOT_SENT]   # WriteBatch's bufs, as wire indexes
    bufs = [b.lens[i] for i in sent]
    addrs = [res[i][2] for i in sent]
    gso = b.max_segments > 1
    iov, entries = [], []
    wire_entry = [NONE] * n
    status = [r[0] for r in res]
    i = 0
    while i < len(bufs):
        entry, iov_idx = 0, 0
        while i < len(bufs):
            budget = b.chunk_packets - iov_idx if b.chunk_packets else len(bufs) + 1
            if budget < 1:
                break
            run, seg = _plan_run(bufs, addrs, i, budget, gso, b.max_segments)
            if run == 0:
                break
            if status[sent[i]] != OK:   # writeSockaddr refuses: the run is skipped, no budget used
                i += run
                continue
            first = len(iov)
            for k in range(run):
                w = sent[i + k]
                iov.append((b.out_off[w], b.lens[w], w))
                wire_entry[w] = len(entries)
            entries.append((first, run, seg if run >= 2 else 0, res[sent[i]][1], sum(bufs[i:i + run])))
            i += run
            iov_idx += run
            entry += 1
        if entry == 0:
            break
    return Plan(iov, entries, wire_entry, status)


# ---- the parallel model ------------------------------------------------------------------------------

IDENT, ZERO = (0, 1), (0, 0)


def _compose(x, y):
    """x first, then y."""
    return (y[x[0]], y[x[1]])


def parallel(b: Batch, detail: dict | None = None) -> Plan:
    res = resolve(b)
    n = len(b.lens)
    status = [r[0] for r in res]
    ms = max(b.max_segments, 1)
    # prefix passes: the previous wire that is not NOT_SENT; the exclusive count of routable wires
    prev, rank = [None] * n, [0] * n
    last, cnt = None, 0
    for i in range(n):
        prev[i], rank[i] = last, cnt
        if status[i] != NOT_SENT:
            last = i
        if status[i] == OK:
            cnt += 1
    nroutable = cnt

    def hard(i):
        p = prev[i]
        if p is None or res[p][2] != res[i][2]:
            return True
        lp, li = b.lens[p], b.lens[i]
        if li == 0 or lp == 0 or lp > MAX_BYTES or li > lp:
            return True
        return bool(b.chunk_packets) and rank[i] // b.chunk_packets != rank[p] // b.chunk_packets

    r_wires = [i for i in range(n) if status[i] == OK]
    is_hard = {i: hard(i) for i in r_wires}
    # plateaus: [first rank, wires, hard]
    plateaus = []
    for i in r_wires:
        if is_hard[i] or b.lens[i] != b.lens[prev[i]]:
            plateaus.append([i, [], is_hard[i]])
        plateaus[-1][1].append(i)

    def cap(z):
        return 1 if z == 0 or z > MAX_BYTES else min(ms, MAX_BYTES // z)

    # plateau j -> the function o_j -> o_{j+1}, placed in front of plateau j + 1
    fns = []
    for j, (first, wires, hd) in enumerate(plateaus):
        if hd:
            fns.append(ZERO)
            continue
        pw = plateaus[j - 1][1]
        z, nj, zn = b.lens[pw[0]], len(pw), b.lens[first]
        f = []
        for o in (0, 1):
            m = nj - o
            if m == 0:
                f.append(0)
                continue
            c = (m - 1) % cap(z) + 1
            f.append(1 if c < ms and c * z + zn <= MAX_BYTES else 0)
        fns.append(tuple(f))
    # the inclusive scan under composition; applied to 0
    o_of, acc = [], IDENT
    for f in fns:
        acc = _compose(acc, f)
        o_of.append(acc[0])
    # run starts -> entry index (a prefix sum), then everything element-wise
    start_of = {}
    for j, (first, wires, hd) in enumerate(plateaus):
        k, o = cap(b.lens[first]), o_of[j]
        for t, w in enumerate(wires):
            start_of[w] = t >= o and (t - o) % k == 0
    wire_entry = [NONE] * n
    firsts = []
    for w in r_wires:
        if start_of[w]:
            firsts.append(w)
        wire_entry[w] = len(firsts) - 1
    iov = [(b.out_off[w], b.lens[w], w) for w in r_wires]
    entries = []
    for e, w in enumerate(firsts):
        first = rank[w]
        end = rank[firsts[e + 1]] if e + 1 < len(firsts) else nroutable
        cntv = end - first
        entries.append((first, cntv, b.lens[w] if cntv >= 2 else 0, res[w][1], sum(x[1] for x in iov[first:end])))
    if detail is not None:
        detail.update(hard=[i for i in r_wires if is_hard[i]], plateaus=[(p[1], p[2]) for p in plateaus], o=o_of,
                      fns=fns, rank=rank, prev=prev)
    return Plan(iov, entries, wire_entry, status)
