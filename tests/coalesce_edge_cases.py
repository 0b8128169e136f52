"""TEST INFRASTRUCTURE ONLY: directed batches at the edges of the plan the receive coalescer's device
form follows (nebula_amd/csrc/coalesce.hip), for tests/test_coalesce_edge_cases.py
(the conditions these cases claim, on the CPU) and tests/test_gpu_coalesce_edges.py (the device).

  sort_*    64-bit counters and epochs whose order hangs on one high bit; ties
  jump_*    runs whose seed count needs every pointer-jumping round the device launches
  gather_*  copies at every (destination, source) residue mod 16 and every split of head, blocks, tail
  rule_*    what only the plan's own keys tell apart: the lane bit of the flow sort, the family, the
            oversize seed as a sealing packet, sealers right after a capped chain, barriers per lane

Every case is deterministic and built from coalesce_ref's packet builders. A packet may carry "pad":
filler bytes in front of its record in the input arena (coalesce_cases.stage_padded)."""
import functools
import random

import coalesce_cases as K
import coalesce_ref as M
from coalesce_cases import P

U64 = (1 << 64) - 1
SPECIAL = (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 48, (1 << 63) - 1, 1 << 63, U64)
JUMP_N = (1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1024, 1025, 4096, 4097)
HALF_N = 1024  # the batch of the S = n/2 + 1 and S = n/2 runs
GATHER_ODD, GATHER_EVEN = (1, 3, 15, 17, 31, 33, 47, 257, 289), (2, 16, 32)
GATHER_OTHER = (1, 17, 33, 257)  # the sizes of the other three header lengths
HDR = dict(tcp4=40, udp4=28, tcp6=60, udp6=48)
_PAT = bytes((7 * i) & 0xFF for i in range(256))


def body(n, tag=0):
    """coalesce_cases.pay without the per-byte loop (the pattern has period 256)."""
    return (_PAT * (n // 256 + 2))[tag & 0xFF:(tag & 0xFF) + n]


def member(kind, i, g, sport, n=None, flags=M.ACK, seq0=1000):
    """Segment i of a flow of `kind` with segment size g (n: this segment's own payload length)."""
    data = body(g if n is None else n, i)
    if kind == "tcp4":
        return M.tcp4(K.A, K.B, sport, 80, seq0 + i * g, data, flags, ident=(100 + i) & 0xFFFF)
    if kind == "tcp6":
        return M.tcp6(K.A6, K.B6, sport, 80, seq0 + i * g, data, flags)
    if kind == "udp4":
        return M.udp4(K.A, K.B, sport, 53, data, ident=(300 + i) & 0xFFFF)
    return M.udp6(K.A6, K.B6, sport, 53, data)


def at_residues(packets, residues):
    """Give every packet the pad that puts its record at residues[i] mod 16 of the input arena."""
    off = K.STAGE_LEAD
    for p, r in zip(packets, residues):
        p["pad"] = (r - off) % 16
        off += p["pad"] + len(p["data"])
    return packets


def shuffled(packets, seed):
    out = list(packets)
    random.Random(seed).shuffle(out)
    return out


# ---- sort keys -------------------------------------------------------------------------------------
def sort_cases():
    c = []
    by_ctr = [P(K.seg(i, size=100), 1 << i) for i in range(64)]
    by_epoch = [P(K.seg(i, size=100), 64 - i, epoch=1 << i) for i in range(64)]  # the counter alone would reverse it
    c.append(("sort_counter_pow2_reversed", by_ctr[::-1]))
    c.append(("sort_counter_pow2_shuffled", shuffled(by_ctr, 1)))
    c.append(("sort_epoch_pow2_reversed", by_epoch[::-1]))
    c.append(("sort_epoch_pow2_shuffled", shuffled(by_epoch, 2)))
    keys = sorted((e, x) for e in SPECIAL for x in SPECIAL)
    spec = []
    for j, (e, x) in enumerate(keys):  # three interleaved flows, each over every (epoch, counter) pair
        spec += [P(K.seg(j, size=100, sport=1000 + f), x, epoch=e) for f in range(3)]
    c.append(("sort_special_values", shuffled(spec, 3)))
    c.append(("sort_tie_whole_flow", [P(K.seg(i, size=100), 7, epoch=7) for i in range(40)]))
    pair = []
    for i in range(20):  # two flows tied pairwise; which of the pair comes first in the input alternates
        two = [P(K.seg(i, size=100, sport=1000), i + 1), P(K.seg(i, size=100, sport=1001), i + 1)]
        pair += two if i % 2 else two[::-1]
    c.append(("sort_tie_two_flows_pairwise", pair))
    c.append(("sort_tie_at_max", [P(K.seg(i, size=100), U64, epoch=U64) for i in range(10)]))
    return c


# ---- pointer jumping -------------------------------------------------------------------------------
def psh_flow(n, sport=1000, size=64):
    """n TCP segments that all carry PSH: every one seeds, closes at once and links to the next."""
    return [K.seg(i, size=size, sport=sport, flags=M.ACK | M.PSH, ident=i & 0xFFFF) for i in range(n)]


def half_batch(seeds, n=HALF_N):
    """One run of `seeds` seeds in n packets; the rest ICMP passthrough, skipped records and a short flow."""
    run = psh_flow(seeds)
    rest = n - seeds
    other = [M.icmp4(K.A, K.B, i, body(24 + i % 40, i)) for i in range(rest - rest // 4 - 11)]
    other += [None] * (rest // 4)  # skipped records
    other += [K.seg(i, size=200, sport=1001) for i in range(11)]
    other = shuffled(other[:-11], 4) + other[-11:]
    out, a, b = [], 0, 0
    for j in range(n):  # the run's packets at the even places while they last
        take_run = a < len(run) and (j % 2 == 0 or b >= len(other))
        d = run[a] if take_run else other[b]
        a, b = (a + 1, b) if take_run else (a, b + 1)
        out.append(P(b"", j + 1, flags=M.PLAIN_SKIP) if d is None else P(d, j + 1))
    assert len(out) == n and a == len(run) and b == len(other)
    return out


def jump_cases():
    c = []
    for n in JUMP_N:
        c.append((f"jump_psh_{n}", K.seq_(psh_flow(n))))
    for n in JUMP_N:  # datagram sizes grow by one: larger than the seed, so every datagram reseeds
        c.append((f"jump_udp_{n}", K.seq_([member("udp4", i, 0, 2000, n=1 + i) for i in range(n)])))
    c.append(("jump_half_plus_one", half_batch(HALF_N // 2 + 1)))
    c.append(("jump_half", half_batch(HALF_N // 2)))
    alt = []
    for r in range(20):  # chains of 64 segments and single PSH packets, alternating, in one run
        alt += [K.seg(65 * r + i, size=50, ident=(65 * r + i) & 0xFFFF) for i in range(64)]
        alt.append(K.seg(65 * r + 64, size=50, flags=M.ACK | M.PSH, ident=(65 * r + 64) & 0xFFFF))
    c.append(("jump_alternating_chain_and_psh", K.seq_(alt)))
    return c


# ---- gather ----------------------------------------------------------------------------------------
def gather_flows(kind, sizes):
    """Per size g: 16 flows of 16 segments, member k of every flow in turn; flow a's records at residue a."""
    pk, res = [], []
    for gi, g in enumerate(sizes):
        for k in range(16):
            for a in range(16):
                pk.append(member(kind, k, g, 3000 + 16 * gi + a))
                res.append(a)
    return at_residues(K.seq_(pk), res)


def gather_cases():
    c = [("gather_tcp4", gather_flows("tcp4", GATHER_ODD + GATHER_EVEN))]
    c += [(f"gather_{kind}", gather_flows(kind, GATHER_OTHER)) for kind in ("udp4", "tcp6", "udp6")]
    pk, res = [], []
    for t in range(1, 16):  # chains that end in a short last segment of t bytes
        for kind in ("tcp4", "udp4"):
            pk += [member(kind, i, 40, 3500 + t) for i in range(3)] + [member(kind, 3, 40, 3500 + t, n=t)]
            res += [t] * 4
    c.append(("gather_short_last", at_residues(K.seq_(pk), res)))
    pk, res = [], []
    for r in range(16):  # verbatim copies at every source residue
        pk.append(P(M.icmp4(K.A, K.B, r, body(20 + 3 * r, r)), 3 * r + 1))
        pk.append(P(b"\xAB", 3 * r + 2, flags=M.PLAIN_PARSED, proto=M.ICMP, ip_hdr_len=20))
        pk.append(P(member("tcp4", 0, 30 + r, 3600 + r), 3 * r + 3))  # a single-segment "chain"
        res += [r] * 3
    c.append(("gather_verbatim", at_residues(pk, res)))
    return c


# ---- rules that only the plan distinguishes -----------------------------------------------------------
BIG = 65500  # payload of the oversize seed: 60 + 65500 (TCP) and 48 + 65500 (UDP) are above 65535


def oversize(kind, where, flags=M.ACK):
    f = [member(kind, i, 100, 4000) for i in range(4)]
    big = member(kind, 9, BIG, 4000, flags=flags)
    return K.seq_(dict(before=[big, f[0], f[1]], between=[f[0], f[1], big, f[2], f[3]], after=[f[0], f[1], big])[where])


def after_cap(kind, size, count, sealer, takes_seq):
    """`count` segments of `size` (a chain closed by a cap), the sealer, three more segments whose
    sequence numbers go on from the last bytes sent, so nothing but the sealer and the cap part them."""
    flow = [member(kind, i, size, 4100) for i in range(count + 4)]
    return K.seq_(flow[:count] + [sealer(count, size)] + flow[count + takes_seq:count + takes_seq + 3])


SEALERS = dict(  # (kind, the packet at the place of segment i, whether it takes segment i's bytes)
    fin=("tcp4", lambda i, g: member("tcp4", i, g, 4100, flags=M.ACK | M.FIN), 1),
    ack=("tcp4", lambda i, g: member("tcp4", i, g, 4100, n=0), 0),
    unparse=("tcp4", lambda i, g: M.tcp4(K.A, K.B, 4100, 80, 1000 + i * g, body(g, i), ident=100 + i, mf=True), 1),
    udp0=("udp4", lambda i, g: member("udp4", i, g, 4100, n=0), 0),
)
CAPS = dict(segcap=dict(tcp4=(100, 64), udp4=(100, 64)), bytecap=dict(tcp4=(1300, 50), udp4=(1400, 46)))


def rule_cases():
    c = []
    both = []
    for i in range(6):  # the flow key has no protocol in it: only the lane keeps these apart
        both += [M.tcp4(K.A, K.B, 5000, 80, 1000 + 100 * i, body(100, i), ident=100 + i),
                 M.udp4(K.A, K.B, 5000, 80, body(100, i), ident=300 + i)]
    c.append(("rule_tcp_udp_same_tuple", K.seq_(both)))
    fam = []
    for i in range(6):  # the v6 addresses are the v4 ones followed by zeros, as the 38-byte key pads them
        fam += [M.tcp4(K.A, K.B, 5001, 80, 1000 + 100 * i, body(100, i), ident=100 + i),
                M.tcp6(K.A + bytes(12), K.B + bytes(12), 5001, 80, 1000 + 100 * i, body(100, i))]
    c.append(("rule_family_only", K.seq_(fam)))
    for kind in ("tcp6", "udp6"):
        for where in ("before", "between", "after"):
            c.append((f"rule_oversize_{kind}_{where}", oversize(kind, where)))
    c.append(("rule_oversize_tcp6_psh", oversize("tcp6", "between", M.ACK | M.PSH)))
    for cap, geo in CAPS.items():
        for nm, (kind, sealer, takes_seq) in SEALERS.items():
            c.append((f"rule_after_{cap}_{nm}", after_cap(kind, *geo[kind], sealer, takes_seq)))
    bad_udp = bytearray(member("udp4", 9, 100, 5003))
    bad_udp[24:26] = (4).to_bytes(2, "big")  # UDP length < 8: unparseable in the UDP lane
    t = [member("tcp4", i, 100, 5002) for i in range(4)]
    u = [member("udp4", i, 100, 5003) for i in range(4)]
    bad_tcp = M.tcp4(K.A, K.B, 5009, 80, 1, body(100), ident=1, mf=True)
    c.append(("rule_barrier_in_other_lane", K.seq_([t[0], t[1], bytes(bad_udp), t[2], t[3], u[0], u[1], bad_tcp, u[2],
                                                    u[3]])))
    return c


@functools.lru_cache(maxsize=None)
def all_cases():
    """[(name, packets, lanes)], built once: read, never changed."""
    return [(name, pk, K.BOTH) for name, pk in sort_cases() + jump_cases() + gather_cases() + rule_cases()]


def family(cases, prefix):
    return [c for c in cases if c[0].startswith(prefix + "_")]


def large_small_large(cases):
    """The cases ordered so that sizes alternate large, small, large: stale workspace beyond n."""
    by = sorted(cases, key=lambda c: len(c[1]))
    out = []
    while by:
        out.append(by.pop())
        if by:
            out.append(by.pop(0))
    return out
