"""TEST INFRASTRUCTURE ONLY: a CPU model of the plan the receive coalescer's device form follows
(nebula_amd/csrc/coalesce.hip), stage by stage between parse and emit, over
coalesce_ref's parsers and rules. It is not a second sequential walk: nothing here keeps a map of
open chains. The stages are the kernel's: the stable order by (epoch, counter, input index), the
per-lane barrier counts, the flow order with each packet's nearest earlier packet of the same
38-byte key, the link bit between neighbours, every data packet's hypothetical chain, next_seed,
pointer jumping, and the slots and write order that follow.

The pointer jumping is synchronous: a round reads only the marks of earlier rounds. The kernel marks
in place, so a thread may see a mark of its own round; that can only mark a seed earlier, so the
synchronous form is the weakest ordering the kernel may see, and the round in which it first marks a
seed is the latest round in which the kernel may.

plan(...) returns the (writes, pkt_write, pkt_status) triple of coalesce_ref.coalesce and a dict of
diagnostics. The product never imports this module."""
import os
import re

import coalesce_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNPARSE, SEAL, ACK, DATA, PASS = range(5)  # the class of a packet in its lane (coalesce_core.hpp)
NONE = None
M32 = 0xFFFFFFFF


def _source():
    return open(os.path.join(ROOT, "nebula_amd", "csrc", "coalesce.hip")).read()


def jump_rounds(n, text=None):
    """The number of co_jump_kernel launches neb_co_run makes for n packets, from the loop as the
    source states it. The loop's form is matched exactly: a changed loop fails here, it is not guessed."""
    text = _source() if text is None else text
    m = re.search(r"for \(uint32_t span = (\d+); span < n; span <<= (\d+)\) \{\s*"
                  r"hipLaunchKernelGGL\(co_jump_kernel, grid, tpb, 0, s, n, jin, jout, ws->reach\);\s*"
                  r"std::swap\(jin, jout\);\s*\}", text)
    assert m, "neb_co_run's pointer-jumping loop no longer has the form this model restates"
    span, shift, rounds = int(m.group(1)), int(m.group(2)), 0
    assert span >= 1 and shift >= 1
    while span < n:
        rounds += 1
        span <<= shift
    return rounds


def gather_lanes(text=None):
    """kCoGatherLanes, and that the gather kernel's split still has the form gather_split restates."""
    text = _source() if text is None else text
    lanes = int(re.search(r"constexpr uint32_t kCoGatherLanes = (\d+);", text).group(1))
    for line in ("const uint32_t head = min(L, (16u - ((uint32_t)reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);",
                 "const uint32_t nb = (L - head) / 16u;",
                 "const bool src_aligned = ((uint32_t)reinterpret_cast<uintptr_t>(sb) & 15u) == 0u;",
                 "const uint32_t t0 = head + 16u * nb;",
                 "for (uint32_t c = l; c < nb; c += kCoGatherLanes) db[c] = s4[c];"):
        assert line in text, f"co_gather_kernel no longer states: {line}"
    return lanes


def gather_split(dst, src, length):
    """One copy as co_gather_kernel splits it: (head bytes, 16-byte blocks, aligned source, tail bytes)."""
    head = min(length, (16 - (dst & 15)) & 15)
    nb = (length - head) // 16
    return head, nb, ((src + head) & 15) == 0, length - head - 16 * nb


def flow_hash(pkt, info):
    """co_flow_hash: groups and orders, never decides equality."""
    h = 0x811C9DC5 ^ int(info["v6"])
    for i in (range(8, 40) if info["v6"] else range(12, 20)):
        h = ((h ^ pkt[i]) * 0x01000193) & M32
    for i in range(4):
        h = ((h ^ pkt[info["ip_hdr_len"] + i]) * 0x01000193) & M32
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M32
    return h ^ (h >> 12)


_TCP, _UDP = M.TCPCoalescer(M.LANE_TCP), M.UDPCoalescer(M.LANE_UDP)


def classify(p, lanes):
    """co_classify -> (status, lane, class, info or None)."""
    fl = p.get("flags", 0)
    if fl & M.PLAIN_SKIP:
        return M.ST_SKIP, M.LANE_PT, PASS, None
    d = p["data"]
    if fl & M.PLAIN_PARSED:
        if len(d) == 0:
            return M.ST_INVALID, M.LANE_PT, PASS, None
        proto, frag_any, ip = p["proto"], bool(fl & M.PLAIN_FRAG_ANY), p["ip_hdr_len"]
    else:
        pp = M.new_packet(d)
        if pp is None:
            return M.ST_INVALID, M.LANE_PT, PASS, None
        proto, frag_any, ip = pp
    if proto == M.TCP and lanes & M.COALESCE_TCP:
        lane, co = M.LANE_TCP, _TCP
    elif proto == M.UDP and lanes & M.COALESCE_UDP:
        lane, co = M.LANE_UDP, _UDP
    else:
        return M.ST_OK, M.LANE_PT, PASS, None
    info = None if frag_any else co.parse_at(d, ip)
    if info is None:
        return M.ST_OK, lane, UNPARSE, None
    info.setdefault("seq", 0)
    info["ip_id"] = 0 if info["v6"] else int.from_bytes(d[4:6], "big")
    info["df"] = (not info["v6"]) and bool(d[6] & 0x40)
    if lane == M.LANE_TCP:
        f = info["flags"]
        if not f & M.ACK or f & ~(M.ACK | M.PSH | M.ECE) & 0xFF:
            return M.ST_OK, lane, SEAL, info
        if info["pay_len"] == 0:
            return M.ST_OK, lane, ACK, info
    elif info["pay_len"] == 0:
        return M.ST_OK, lane, SEAL, info
    if info["hdr_len"] + info["pay_len"] > M.BUF_SIZE:  # the oversize seed: never appends, always seals
        return M.ST_OK, lane, SEAL, info
    return M.ST_OK, lane, DATA, info


def neighbour_link(p, ip, q, iq, tcp):
    """co_link: canAppend's comparisons between two consecutive data packets p then q of one flow."""
    if ip["hdr_len"] != iq["hdr_len"] or ip["v6"] != iq["v6"]:
        return False
    if tcp and iq["seq"] != (ip["seq"] + ip["pay_len"]) & M32:
        return False
    if tcp and (ip["flags"] ^ iq["flags"]) & M.ECE:
        return False
    if not ip["v6"] and not ip["df"] and iq["ip_id"] != (ip["ip_id"] + 1) & 0xFFFF:
        return False
    co = _TCP if tcp else _UDP
    return co.headers_match(p[:ip["hdr_len"]], q[:iq["hdr_len"]], ip["v6"], ip["ip_hdr_len"])


def plan(packets, lanes=M.COALESCE_TCP | M.COALESCE_UDP, out_cap=1 << 62, max_writes=1 << 31, rounds=None,
         hash_bits=32):
    """-> ((writes, pkt_write, pkt_status), diagnostics). rounds=None: as many as neb_co_run launches."""
    n = len(packets)
    R = jump_rounds(n)
    rounds = R if rounds is None else rounds
    rec = [classify(p, lanes) for p in packets]
    # sort: stable by counter, then stable by epoch; the position is "time" for everything below
    order = sorted(range(n), key=lambda i: packets[i]["counter"])
    order.sort(key=lambda i: packets[i]["epoch"])
    st = [rec[i][0] for i in order]
    lane = [rec[i][1] for i in order]
    cls = [rec[i][2] for i in order]
    info = [rec[i][3] for i in order]
    data = [packets[i].get("data", b"") for i in order]
    live = [st[pos] == M.ST_OK and lane[pos] != M.LANE_PT for pos in range(n)]
    # barriers: per lane, the inclusive count of unparseable packets
    bar, cnt = [], [0, 0]
    for pos in range(n):
        if live[pos] and cls[pos] == UNPARSE:
            cnt[lane[pos]] += 1
        bar.append(tuple(cnt))
    # flows: stable sort of the data and sealing packets by (lane, hash); walk back through the hash
    # group to the nearest packet with the same 38-byte key
    mask = M32 if hash_bits >= 32 else (1 << hash_bits) - 1
    inflow = [pos for pos in range(n) if live[pos] and cls[pos] in (DATA, SEAL)]
    fkey = {pos: (lane[pos], flow_hash(data[pos], info[pos]) & mask) for pos in inflow}
    forder = sorted(inflow, key=lambda pos: fkey[pos])
    fprev, fnext = [NONE] * n, [NONE] * n
    for j, pos in enumerate(forder):
        for jj in range(j - 1, -1, -1):
            pos2 = forder[jj]
            if fkey[pos2] != fkey[pos]:
                break
            if info[pos2]["fk"] == info[pos]["fk"]:
                fprev[pos], fnext[pos2] = pos2, pos
                break
    # links
    isdata = [live[pos] and cls[pos] == DATA for pos in range(n)]
    link = [False] * n
    for pos in range(n):
        pp = fprev[pos]
        if isdata[pos] and pp is not NONE and isdata[pp] and bar[pp][lane[pos]] == bar[pos][lane[pos]]:
            link[pos] = neighbour_link(data[pp], info[pp], data[pos], info[pos], lane[pos] == M.LANE_TCP)
    reach = [isdata[pos] and not link[pos] for pos in range(n)]
    psh = [isdata[pos] and lane[pos] == M.LANE_TCP and bool(info[pos]["flags"] & M.PSH) for pos in range(n)]
    # chains: every data packet as a hypothetical seed
    jump, cnseg, ctotal, cpsh = list(range(n)), [0] * n, [0] * n, [False] * n
    for pos in range(n):
        if not isdata[pos]:
            continue
        hdr, gso = info[pos]["hdr_len"], info[pos]["pay_len"]
        nseg, total, closed, last, q = 1, gso, psh[pos], pos, fnext[pos]
        while not closed and q is not NONE and link[q]:
            pl = info[q]["pay_len"]
            if nseg >= M.MAX_SEGS or pl > gso or hdr + total + pl > M.BUF_SIZE:
                break
            nseg, total, last = nseg + 1, total + pl, q
            cpsh[pos] = cpsh[pos] or psh[q]
            closed = pl < gso or psh[q]
            q = fnext[q]
        nx = fnext[last]
        if nx is not NONE and link[nx]:
            jump[pos] = nx
        cnseg[pos], ctotal[pos] = nseg, total
    # the runs, for the diagnostics: the seeds reachable from each run's first packet
    run_seeds = []
    for pos in range(n):
        if reach[pos]:
            s, q = 1, pos
            while jump[q] != q:
                q, s = jump[q], s + 1
            run_seeds.append(s)
    # pointer jumping, synchronous
    first_round = {pos: 0 for pos in range(n) if reach[pos]}
    for r in range(1, rounds + 1):
        new = list(reach)
        for pos in range(n):
            j = jump[pos]
            if j != pos and reach[pos] and not new[j]:
                new[j] = True
                first_round[j] = r
        jump = [jump[jump[pos]] for pos in range(n)]
        reach = new
    # members of the real seeds' chains; slot-creating positions per lane
    mseed, midx = [NONE] * n, [0] * n
    slots = [[], [], []]
    for pos in range(n):
        if st[pos] != M.ST_OK:
            continue
        if isdata[pos]:
            if not reach[pos]:
                continue
            q = pos
            for k in range(cnseg[pos]):
                if q is NONE:
                    break
                mseed[q], midx[q] = pos, k
                q = fnext[q]
        slots[lane[pos]].append(pos)
    wpos = slots[0] + slots[1] + slots[2]
    wk = {pos: k for k, pos in enumerate(wpos)}
    wsize = [M.align16(info[pos]["hdr_len"] + ctotal[pos] if isdata[pos] and cnseg[pos] >= 2 else len(data[pos]))
             for pos in wpos]
    woff, acc = [0] * len(wpos), 0
    for k, sz in enumerate(wsize):
        woff[k], acc = acc, acc + sz
    fits = [k < max_writes and woff[k] + wsize[k] <= out_cap for k in range(len(wpos))]
    nwrites = 0
    while nwrites < len(wpos) and fits[nwrites]:
        nwrites += 1
    assert not any(fits[nwrites:]), "the fitting writes are a prefix"
    # per-packet results and the copies the gather makes
    pkt_write, pkt_status, copies = [M.WRITE_NONE] * n, [M.ST_OK] * n, [None] * n
    members = {}
    for pos in range(n):
        i = order[pos]
        pkt_status[i] = st[pos]
        if st[pos] != M.ST_OK:
            continue
        spos = mseed[pos] if isdata[pos] else pos
        k = wk.get(spos) if spos is not NONE else None
        if k is None or not fits[k]:
            pkt_status[i] = M.ST_NO_SPACE
            continue
        pkt_write[i] = k
        members.setdefault(k, []).append(pos)
        if isdata[pos] and cnseg[spos] >= 2:
            copies[i] = (info[pos]["hdr_len"], woff[k] + info[spos]["hdr_len"] + midx[pos] * info[spos]["pay_len"],
                         info[pos]["pay_len"])
        else:
            copies[i] = (0, woff[k], len(data[pos]))
    # the writes
    w = M.Writer()
    for k in range(nwrites):
        pos = wpos[k]
        if not (isdata[pos] and cnseg[pos] >= 2):
            w.Write(data[pos], order[pos], lane[pos])
            continue
        mem = sorted(members[k], key=lambda q: midx[q])
        s = M._Slot()
        s.hdr = bytearray(data[pos][:info[pos]["hdr_len"]])
        if cpsh[pos]:
            s.hdr[info[pos]["ip_hdr_len"] + 13] |= M.PSH
        s.hdr_len, s.ip_hdr_len, s.v6, s.total_pay = (info[pos]["hdr_len"], info[pos]["ip_hdr_len"], info[pos]["v6"],
                                                      ctotal[pos])
        s.pays = [data[q][info[q]["hdr_len"]:info[q]["hdr_len"] + info[q]["pay_len"]] for q in mem]
        s.first, s.members = order[pos], [order[q] for q in mem]
        (_TCP if lane[pos] == M.LANE_TCP else _UDP).flush_slot(s, w)
    writes = [dict(wr, out_off=woff[k], len=len(wr["data"]), nseg=len(wr["members"])) for k, wr in enumerate(w.writes)]
    diag = dict(R=R, rounds=rounds, order=order, run_seeds=run_seeds,
                first_round={order[pos]: r for pos, r in first_round.items()},
                link={order[pos]: link[pos] for pos in range(n)}, copies=copies)
    return (writes, pkt_write, pkt_status), diag
