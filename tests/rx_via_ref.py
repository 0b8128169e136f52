"""TEST INFRASTRUCTURE ONLY: two sequential models of a node that receives through relays, for
tests/test_rx_via_model.py and tests/test_gpu_rx_via.py.

Per datagram, as readOutsidePackets does (outside.go:30-133): the gate
(replay_oracle.read_outside_gate), then Check -> Decrypt or VerifyRelay -> Update
(replay_oracle.rx_sequential, one packet at a time). A verified Message/Relay datagram whose relay
is a TerminalType is unwrapped (handleOutsideRelayPacket, outside.go:210-219: signedPayload =
packet[16 : len-16]) and readOutsidePackets runs again on the inner packet with IsRelayed = true.

  rx_via_strict    the reference's order: the recursion runs inside the loop, packet by packet.
  rx_via_deferred  the contract of neb_rx_open_via_batch (include/nebula_aead.h): every datagram's
                   own receive first, in arrival order, then the inner packets, in arrival order.

Both stop at one level: an inner packet that is itself Message/Relay gets NOT_MESSAGE and is left
alone. Pure Python over oracle.open_ / nonce and replay_oracle."""
NOT_RELAYED = 9
VIA_TERMINAL = 1
OTHER_ALG = "other-alg"  # keys[t]: the tunnel's key belongs to the other cipher (the open's BAD_KEY)


def seal_message(oracle_mod, alg, key, remote_index, c, pt, typ=1, sub=0):
    hdr = oracle_mod.header_encode(1, typ, sub, remote_index, c)
    return hdr + oracle_mod.seal(alg, key, oracle_mod.nonce(alg, c), hdr, pt)


def seal_relay(oracle_mod, alg, key, remote_index, c, inner):
    """A Message/Relay wire packet: header || inner || tag, the tag over header || inner."""
    ad = oracle_mod.header_encode(1, 1, 1, remote_index, c) + inner
    return ad + oracle_mod.seal(alg, key, oracle_mod.nonce(alg, c), ad, b"")


def unwrap(status, head, off, ln, via):
    """The unwrap rule for one finished outer packet. head: its first two bytes (b"" when it has
    none); via: (inner tunnel or None, flags). Returns (eligible, (off, len, tunnel))."""
    eligible = (status == 0 and ln >= 32 and len(head) >= 2 and head[0] & 15 == 1 and head[1] == 1
                and bool(via[1] & VIA_TERMINAL))
    return (True, (off + 16, ln - 32, via[0])) if eligible else (False, (off, 0, None))


def _receive(oracle_mod, R, alg, keys, wins, exp, off, ln, t, relayed):
    """One readOutsidePackets on exp[off:off+ln] for tunnel t, through wins; opens in place."""
    pkt = bytes(exp[off:off + ln])
    if relayed and ln >= 16 and pkt[0] >> 4 == 1 and pkt[0] & 15 == 1 and pkt[1] == 1:
        return R.NOT_MESSAGE  # a relay inside a relay: the next call's (it passed ver and IsValidSubType)
    st, go = R.read_outside_gate(pkt, t is not None)
    if st is not None:
        return st
    kind, c = go
    key, pt = keys.get(t), None
    if key is None or key == OTHER_ALG:
        verdict = R.BAD_KEY
    elif kind == "relay":
        verdict = oracle_mod.open_(alg, key, oracle_mod.nonce(alg, c), pkt[:ln - 16], pkt[ln - 16:]) is not None
    else:
        pt = oracle_mod.open_(alg, key, oracle_mod.nonce(alg, c), pkt[:16], pkt[16:])
        verdict = pt is not None
    (st,), (decrypted,) = R.rx_sequential(wins, [t], [c], [verdict])
    if decrypted and kind == "decrypt" and verdict is not R.BAD_KEY:
        exp[off + 16:off + ln - 16] = list(pt) if verdict else 0  # a failed open zeroes its destination
    return st


def _run(oracle_mod, R, alg, keys, wins, arena, packets, via, strict):
    exp = arena.copy()
    n = len(packets)
    status, inner, inner_status = [None] * n, [None] * n, [NOT_RELAYED] * n
    todo = []
    for i, (off, ln, t) in enumerate(packets):
        status[i] = _receive(oracle_mod, R, alg, keys, wins, exp, off, ln, t, False)
        ok, inner[i] = unwrap(status[i], bytes(exp[off:off + min(ln, 2)]), off, ln, via[i])
        if ok and strict:
            inner_status[i] = _receive(oracle_mod, R, alg, keys, wins, exp, *inner[i], True)
        elif ok:
            todo.append(i)
    for i in todo:
        inner_status[i] = _receive(oracle_mod, R, alg, keys, wins, exp, *inner[i], True)
    return status, inner, inner_status, exp


def rx_via_deferred(oracle_mod, R, alg, keys, wins, arena, packets, via):
    """keys: {tunnel: key bytes or OTHER_ALG}; wins: {tunnel: Bits}, updated in place; packets:
    [(off, len, tunnel or None)]; via: [(inner tunnel or None, flags)].
    Returns (status, inner packets [(off, len, tunnel or None)], inner_status, expected arena)."""
    return _run(oracle_mod, R, alg, keys, wins, arena, packets, via, False)


def rx_via_strict(oracle_mod, R, alg, keys, wins, arena, packets, via):
    return _run(oracle_mod, R, alg, keys, wins, arena, packets, via, True)


def win_state(w):
    return (w.current, w.lost, w.dupe, w.out_of_window, tuple(w.snapshot()))


def random_batch(oracle_mod, alg, rng, n, nrelay=2, ndirect=2, ntarget=3, terminal=0.9, noise=True, payloads=(0, 1, 20, 100)):
    """A shuffled-in-time receive batch of a node behind relays. Tunnels 0..nrelay-1 are relays,
    the next ndirect are peers heard directly (phase 1 only), the next ntarget are peers heard only
    through a relay (phase 2 only). noise: forged outer and inner packets, replayed datagrams, inner
    packets wrapped twice, short and odd inner packets, inner packets without a tunnel, relay
    packets that are not terminal. Returns (keys {tunnel: key}, [(bytes, outer tunnel)], via)."""
    nt = nrelay + ndirect + ntarget
    keys = {t: bytes(rng.getrandbits(8) for _ in range(32)) for t in range(nt)}
    ctr = [0] * nt
    targets = list(range(nrelay + ndirect, nt))

    def nxt(t):
        ctr[t] += 1 + (rng.random() < 0.1) * rng.randrange(1, 40)
        return ctr[t]

    pkts, via, inners = [], [], []
    while len(pkts) < n:
        r = rng.random() if noise else 0.5
        if r < 0.08 and pkts:  # the same datagram again
            k = rng.randrange(len(pkts))
            pkts.append(pkts[k])
            via.append(via[k])
            continue
        if ndirect and (0.3 < r < 0.45 or not nrelay):  # a peer heard directly
            t = nrelay + rng.randrange(ndirect)
            p = bytearray(seal_message(oracle_mod, alg, keys[t], 0x100 + t, nxt(t), bytes(rng.getrandbits(8) for _ in range(rng.choice(payloads)))))
            if noise and rng.random() < 0.1:
                p[rng.randrange(16, len(p))] ^= 1
            if noise and rng.random() < 0.05:
                p = p[:rng.choice([0, 3, 16, 31])]
            pkts.append((bytes(p), t))
            via.append((rng.choice(targets + [None]), rng.choice([0, VIA_TERMINAL])))  # TERMINAL on a non-relay packet
            continue
        g = rng.choice(targets)
        if r < 0.14 and inners:  # an inner packet seen before, under a new outer counter
            inner, g = rng.choice(inners)
        elif r < 0.2:  # short and odd inner packets
            inner = rng.choice([b"", b"\x11", bytes(15), oracle_mod.header_encode(1, 1, 0, 7, 9), oracle_mod.header_encode(1, 1, 0, 7, 9) + bytes(15),
                                oracle_mod.header_encode(1, 0, 0, 7, 1) + bytes(40), oracle_mod.header_encode(1, 2, 0, 7, 1) + bytes(20),
                                oracle_mod.header_encode(2, 1, 0, 7, 1) + bytes(40), oracle_mod.header_encode(1, 1, 1, 7, 1) + bytes(40)])
        else:
            inner = bytearray(seal_message(oracle_mod, alg, keys[g], 0x100 + g, nxt(g), bytes(rng.getrandbits(8) for _ in range(rng.choice(payloads)))))
            if noise and rng.random() < 0.1:
                inner[rng.randrange(len(inner))] ^= 4  # forged before it was wrapped: the outer tag holds
            inner = bytes(inner)
            inners.append((inner, g))
        t = rng.randrange(nrelay)
        p = bytearray(seal_relay(oracle_mod, alg, keys[t], 0x100 + t, nxt(t), inner))
        if noise and rng.random() < 0.08:
            p[rng.randrange(16, len(p))] ^= 0x20  # forged on the way to us
        pkts.append((bytes(p), t))
        flags = VIA_TERMINAL if rng.random() < terminal else 0
        via.append((None if noise and rng.random() < 0.05 else g, flags))
    return keys, pkts, via


def lay_out(pkts, slot):
    """pkts: [(bytes, tunnel or None)] -> arena (numpy uint8), [(off, len, tunnel)]"""
    import numpy as np

    arena = np.zeros(max(len(pkts), 1) * slot, np.uint8)
    packets = []
    for i, (p, t) in enumerate(pkts):
        arena[i * slot:i * slot + len(p)] = np.frombuffer(p, np.uint8)
        packets.append((i * slot, len(p), t))
    return arena, packets
