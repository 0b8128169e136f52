"""TEST INFRASTRUCTURE ONLY: the sequential model of sendInsideMessage with its relay branch
(inside.go:154-240) over a batch of TUN reads, for tests/test_tx_via_model.py and
tests/test_gpu_tx_via.py.

segment_oracle.tx_batch restated with the relay rules: per read in batch order, per segment in
order, with two live counter arrays. A read whose tunnel t has via[t] = (v, remote index) is
refused with BAD_KEY when no usable relay tunnel v exists (inside.go:195-198) and with INVALID when
v == t or v itself has a via (a relay is always reached directly); otherwise every segment takes
the next counter of t and is sealed under t's key behind header.Encode(Message, 0) at +16 of its
slot (sendInsideEncrypt on scratch[16:], inside.go:199-207), then takes the next counter of v,
gets header.Encode(Message, MessageRelay, via remote index, r) in front and the tag of the AD-only
seal under v's key behind (prepareSendVia, inside.go:442-501). An exhausted inner counter takes no
outer one; an exhausted outer counter is still used. Pure Python over segment_oracle's segmentation
functions and oracle.seal / nonce / header_encode."""
import segment_oracle as S

RELAY_NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def slot_bytes_via(seg_len: int) -> int:
    return (seg_len + 64 + 15) & ~15


def oracle_seal(oracle_mod):
    """The seal callback of segment_oracle.tx_batch and tx_via_batch over the AEAD oracle."""
    return lambda a, key, ctr, ad, pt: oracle_mod.seal(a, key, oracle_mod.nonce(a, ctr), ad, pt)


def tx_via_batch(alg, tunnels, via, packets, out_cap, max_wires, seal, header_encode):
    """tunnels, packets, out_cap, max_wires, seal, header_encode: as segment_oracle.tx_batch;
    via: None, or one (relay tunnel or RELAY_NONE, relay remote index) per tunnel.
    Returns (wires [(off, inner counter, len, packet, segment, status, via flag, bytes or None)],
    packet statuses, final counters)."""
    ctr = [t["counter"] for t in tunnels]
    nt = len(tunnels)

    def relay_of(t):
        return via[t][0] if via is not None and t < nt else RELAY_NONE

    pst, plans, relays = [], [], []
    for p in packets:
        g = p["gso_type"] & ~S.GSO_ECN
        st, segs, hl = S.OK, None, 0
        try:  # read time
            if len(p["data"]) == 0:
                raise S.SegmentError("short read")
            if g == S.GSO_NONE:
                if p["flags"] & S.F_NEEDS_CSUM:
                    segs = [S.finish_checksum(p["data"], p["csum_start"], p["csum_offset"])]
                else:
                    segs = [bytes(p["data"])]
            else:
                S.check_valid(p["data"], p["flags"], p["gso_type"], p["gso_size"])
                hl = S.correct_hdr_len(p["data"], p["gso_type"], p["csum_start"], p["csum_offset"])
                if g not in (S.GSO_TCPV4, S.GSO_TCPV6, S.GSO_UDP_L4):
                    raise S.SegmentError("unsupported gso type")
        except S.SegmentError:
            st = S.INVALID
        t = p["tunnel"]
        if st == S.OK and (t >= nt or tunnels[t]["key"] is None):
            st = S.BAD_KEY
        v = relay_of(t) if st == S.OK else RELAY_NONE
        if v != RELAY_NONE:  # the relay lookup, before SegmentSuperpacket
            if v >= nt or tunnels[v]["key"] is None:
                st = S.BAD_KEY
            elif v == t or relay_of(v) != RELAY_NONE:
                st = S.INVALID
        if st == S.OK and segs is None:
            try:
                fn = S.segment_tcp if g in (S.GSO_TCPV4, S.GSO_TCPV6) else S.segment_udp
                segs = fn(p["data"], hl, p["csum_start"], p["gso_size"])
            except S.SegmentError:
                st = S.INVALID
        pst.append(st)
        plans.append(segs if st == S.OK else [])
        relays.append(v if st == S.OK else RELAY_NONE)
    # fitting prefix
    nw = nb = 0
    fit = len(packets)
    for i, segs in enumerate(plans):
        size = slot_bytes_via if relays[i] != RELAY_NONE else S.slot_bytes
        nw2 = nw + len(segs)
        nb2 = nb + sum(size(len(s)) for s in segs)
        if nw2 > max_wires or nb2 > out_cap:
            fit = i
            break
        nw, nb = nw2, nb2
    wires, off = [], 0
    for i, (p, segs) in enumerate(zip(packets, plans)):
        if i >= fit:
            if pst[i] == S.OK:
                pst[i] = S.NO_SPACE
            continue
        t, v = p["tunnel"], relays[i]
        for j, seg in enumerate(segs):
            ctr[t] = (ctr[t] + 1) & M64
            c = ctr[t]
            hdr = header_encode(1, 1, 0, tunnels[t]["remote_index"], c)
            if v == RELAY_NONE:
                if c >= S.REJECT_AFTER:
                    wires.append((off, c, len(seg) + 32, i, j, S.EXHAUSTED, 0, None))
                else:
                    wires.append((off, c, len(seg) + 32, i, j, S.OK, 0, hdr + seal(alg, tunnels[t]["key"], c, hdr, seg)))
                off += S.slot_bytes(len(seg))
                continue
            data, st = None, S.EXHAUSTED
            if c < S.REJECT_AFTER:  # else sendInsideEncrypt returned nil: prepareSendVia is not reached
                inner = hdr + seal(alg, tunnels[t]["key"], c, hdr, seg)
                ctr[v] = (ctr[v] + 1) & M64
                r = ctr[v]
                if r < S.REJECT_AFTER:
                    ad = header_encode(1, 1, 1, via[t][1], r) + inner
                    data, st = ad + seal(alg, tunnels[v]["key"], r, ad, b""), S.OK
            wires.append((off, c, len(seg) + 64, i, j, st, 1, data))
            off += slot_bytes_via(len(seg))
    return wires, pst, ctr
