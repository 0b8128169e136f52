"""TEST INFRASTRUCTURE ONLY: the sequential model of a relay node's receive loop with forwarding,
for tests/test_relay_forward.py and tests/test_gpu_relay_forward.py.

Per packet in arrival order, as readOutsidePackets does (outside.go:30-133): the gate
(replay_oracle.read_outside_gate), the window Check, Decrypt or VerifyRelay with the inbound key,
the window Update; then, for a verified Message/Relay packet with a route,
handleOutsideRelayPacket's ForwardingType branch (outside.go:220-240): prepareSendVia
(inside.go:442-501) takes the next message counter of the target tunnel, writes
header.Encode(1, Message, MessageRelay, remote index, c) over the old header and the tag of the
AD-only seal under the target key where the old tag was. Pure Python over oracle.seal / open_ /
nonce / header_encode and replay_oracle.Bits."""
NOT_FORWARDED = 8
RELAY_NONE = 0xFFFFFFFF
REJECT_AFTER = (1 << 64) - 1 - (1 << 40)
M64 = (1 << 64) - 1


def seal_relay(oracle_mod, alg, key, remote_index, c, inner):
    """A Message/Relay wire packet: header || inner || tag, the tag over header || inner."""
    ad = oracle_mod.header_encode(1, 1, 1, remote_index, c) + inner
    return ad + oracle_mod.seal(alg, key, oracle_mod.nonce(alg, c), ad, b"")


def seal_message(oracle_mod, alg, key, remote_index, c, pt, typ=1, sub=0):
    hdr = oracle_mod.header_encode(1, typ, sub, remote_index, c)
    return hdr + oracle_mod.seal(alg, key, oracle_mod.nonce(alg, c), hdr, pt)


def forward(oracle_mod, R, alg, keys, arena, packets, routes, tunnels, window_len, seen=(1, 2)):
    """keys[t]: the inbound key of tunnel t; packets: [(off, len, inbound tunnel or None)];
    routes: [(target tunnel or RELAY_NONE, remote_index)]; tunnels: [(message_counter, target key
    or None)]. Every window starts with the counters of `seen` received.
    Returns (status, fwd_status, expected arena, windows {t: Bits}, final message counters)."""
    wins = {t: R.Bits(window_len) for t in range(len(keys))}
    for w in wins.values():
        for c in seen:
            w.update(c)
    ctr = [t[0] for t in tunnels]
    exp = arena.copy()
    status, fwd = [], []
    for (off, ln, t), (rt, ri) in zip(packets, routes):
        pkt = bytes(arena[off:off + ln])
        fwd.append(NOT_FORWARDED)
        st, go = R.read_outside_gate(pkt, t is not None)
        if st is not None:
            status.append(st)
            continue
        kind, c = go
        w = wins[t]
        if not w.check(c):
            status.append(R.REPLAY)
            continue
        nb = oracle_mod.nonce(alg, c)
        if kind == "relay":
            ok = oracle_mod.open_(alg, keys[t], nb, pkt[:ln - 16], pkt[ln - 16:]) is not None
        else:
            pt = oracle_mod.open_(alg, keys[t], nb, pkt[:16], pkt[16:])
            ok = pt is not None
            exp[off + 16:off + ln - 16] = list(pt) if ok else 0
        if not ok:
            status.append(R.AUTH_FAILED)
            continue
        if not w.update(c):
            status.append(R.REPLAY)
            continue
        status.append(R.OK)
        if kind != "relay" or rt == RELAY_NONE:
            continue
        if rt >= len(tunnels) or tunnels[rt][1] is None:
            fwd[-1] = R.BAD_KEY
            continue
        ctr[rt] = (ctr[rt] + 1) & M64  # NextMessageCounter
        n = ctr[rt]
        if n >= REJECT_AFTER:
            fwd[-1] = R.EXHAUSTED  # prepareSendVia returns before Encode
            continue
        out = oracle_mod.header_encode(1, 1, 1, ri, n) + pkt[16:ln - 16]
        out += oracle_mod.seal(alg, tunnels[rt][1], oracle_mod.nonce(alg, n), out, b"")
        exp[off:off + ln] = list(out)
        fwd[-1] = R.OK
    return status, fwd, exp, wins, ctr
