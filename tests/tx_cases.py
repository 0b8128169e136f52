"""TEST INFRASTRUCTURE ONLY: directed TUN reads for the transmit path (nebula_amd/csrc/tx.hip
tx_parse_one and tx_segment_kernel; the seal-side checksum of nebula_amd/csrc/gcm_packet.hpp
gcm_csum_fix), for tests/test_tx_cases.py (CPU) and tests/test_gpu_tx_edges.py (GPU).

Header builders with every field the kernels branch or do arithmetic on as a parameter, payload
generators, steer_zero / steer_ipck_zero (a computed checksum of exactly zero), the named case
lists, and conditions() / uncovered(): what the cases reach, derived from the oracle's plaintext
segments and statuses (oracle/segment_oracle.py) and a restatement of tx.hip's per-segment seal_cs
predicate (the pass rule of a capped seal grid depends on the CU count and is not modelled).

Reads are packet dicts in the form test_gpu_tx._pk makes; every read of a case list carries tunnel 0
and the GPU tests give each case list one tunnel."""
import random
import struct

import segment_oracle as S

CWR, URG, ACK, PSH, SYN, FIN = 0x80, 0x20, 0x10, 0x08, 0x02, 0x01
FLAG_BYTES = {"all": 0xFF, "cwr_ack_psh_fin": CWR | ACK | PSH | FIN, "ack": ACK, "syn_urg": SYN | URG}


def _pk(data, flags=0, gso_type=0, gso_size=0, csum_start=0, csum_offset=0):
    return dict(data=bytes(data), tunnel=0, flags=flags, gso_type=gso_type, hdr_len=0, gso_size=gso_size,
                csum_start=csum_start, csum_offset=csum_offset)


# ---- payloads ---------------------------------------------------------------------------------

def rand_bytes(n, seed):
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little") if n else b""


def ones(n, seed=None):
    return b"\xff" * n


def zeros(n, seed=None):
    return bytes(n)


# ---- headers ----------------------------------------------------------------------------------

def _pattern(n, k):
    return bytes((i * 37 + 11 * k + 5) & 0xFF for i in range(n))


def l3_header(v, proto, ip_opts=0, ident=0x4242, ext=0, gap=0, src=None, dst=None):
    """IPv4 (20 + ip_opts bytes, the ID) or IPv6 (40 bytes + an `ext`-byte destination-options header,
    ext a multiple of 8), then `gap` bytes that belong to neither header: csum_start = its length.
    The length and checksum fields hold values the segmenter must replace."""
    if v == 4:
        ihl = 20 + ip_opts
        h = bytearray(ihl)
        h[0], h[1] = 0x40 | (ihl // 4), 0x1C
        struct.pack_into(">HHH", h, 2, 0xFEDC, ident, 0x4000)
        h[8], h[9] = 64, proto
        struct.pack_into(">H", h, 10, 0xA55A)
        h[12:16], h[16:20] = src or bytes([10, 1, 2, 3]), dst or bytes([172, 16, 254, 9])
        h[20:] = _pattern(ip_opts, 1)
    else:
        h = bytearray(40 + ext)
        h[0:4] = bytes([0x6A, 0xBC, 0xDE, 0xF1])
        struct.pack_into(">H", h, 4, 0xFEDC)
        h[6], h[7] = (60 if ext else proto), 64
        h[8:24] = src or bytes(range(0xE1, 0xF1))
        h[24:40] = dst or bytes([0xFD] + [0xFF] * 14 + [0x02])
        if ext:
            h[40:] = bytes([proto, ext // 8 - 1, 1, ext - 4]) + _pattern(ext - 4, 2)
    return bytes(h) + _pattern(gap, 3)


def tcp_header(opts=0, seq=10000, flags=ACK | PSH, doff=None):
    h = bytearray(20 + opts)
    struct.pack_into(">HHII", h, 0, 0xC001, 443, seq & 0xFFFFFFFF, 0xFFFE0001)
    h[12], h[13] = ((20 + opts if doff is None else doff) // 4) << 4, flags
    struct.pack_into(">HHH", h, 14, 0xFFFF, 0x1234, 0)
    h[20:] = _pattern(opts, 4)
    return bytes(h)


def udp_header():
    return struct.pack(">HHHH", 0xD002, 4242, 0xFEDC, 0x1234)


def tso(v, payload, gso, *, ip_opts=0, ident=0x4242, tcp_opts=0, seq=10000, flags=ACK | PSH, ext=0, gap=0, ecn=False,
        src=None):
    l3 = l3_header(v, 6, ip_opts, ident, ext, gap, src)
    g = (S.GSO_TCPV4 if v == 4 else S.GSO_TCPV6) | (S.GSO_ECN if ecn else 0)
    return _pk(l3 + tcp_header(tcp_opts, seq, flags) + payload, S.F_NEEDS_CSUM, g, gso, len(l3), 16)


def uso(v, payload, gso, *, ip_opts=0, ident=0x4242, ext=0, gap=0, src=None):
    l3 = l3_header(v, 17, ip_opts, ident, ext, gap, src)
    return _pk(l3 + udp_header() + payload, S.F_NEEDS_CSUM, S.GSO_UDP_L4, gso, len(l3), 6)


def _fold(s):
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def finish_l4(v, proto, payload, **kw):
    """One whole TCP or UDP packet as the kernel hands it over with NEEDS_CSUM: the checksum field
    holds the folded pseudo-header sum."""
    l3 = bytearray(l3_header(v, proto, **kw))
    l4 = bytearray(tcp_header() if proto == 6 else udp_header())
    n = len(l4) + len(payload)
    if proto == 17:
        struct.pack_into(">H", l4, 4, n)
    if v == 4:
        struct.pack_into(">H", l3, 2, len(l3) + n)
        addrs = l3[12:20]
    else:
        struct.pack_into(">H", l3, 4, len(l3) - 40 + n)
        addrs = l3[8:40]
    co = 16 if proto == 6 else 6
    struct.pack_into(">H", l4, co, _fold(sum(struct.unpack(f">{len(addrs) // 2}H", addrs)) + proto + n))
    return _pk(bytes(l3) + bytes(l4) + payload, S.F_NEEDS_CSUM, 0, 0, len(l3), co)


def finish_raw(data, cs, co):
    return _pk(data, S.F_NEEDS_CSUM, 0, 0, cs, co)


def plain(data):
    return _pk(data)


# ---- the oracle's view of one read ------------------------------------------------------------

def read_result(pk):
    """(status, plaintext segments) as segment_oracle.tx_batch decides them for a keyed tunnel."""
    if len(pk["data"]) == 0:
        return S.INVALID, []
    try:
        return S.OK, S.segment_superpacket(pk["data"], pk["flags"], pk["gso_type"], pk["hdr_len"], pk["gso_size"],
                                           pk["csum_start"], pk["csum_offset"])
    except S.SegmentError:
        return S.INVALID, []


def kind_of(pk):
    g = pk["gso_type"] & ~S.GSO_ECN
    if g == S.GSO_NONE:
        return "finish" if pk["flags"] & S.F_NEEDS_CSUM else "pass"
    return {S.GSO_TCPV4: "tcp", S.GSO_TCPV6: "tcp", S.GSO_UDP_L4: "udp"}.get(g, "unknown")


def field_of(pk):
    """Offset of the L4 checksum field in every segment of the read."""
    k = kind_of(pk)
    return pk["csum_start"] + (16 if k == "tcp" else 6 if k == "udp" else pk["csum_offset"])


def hdr_len_of(pk):
    return S.correct_hdr_len(pk["data"], pk["gso_type"], pk["csum_start"], pk["csum_offset"])


# ---- steering a computed checksum to zero -----------------------------------------------------

def _steer_pos(pk, hl, j):
    if kind_of(pk) != "finish":
        return hl + j * pk["gso_size"]  # the segment's first payload word: hl - cs is even
    cs, co = pk["csum_start"], pk["csum_offset"]
    k = co + 2 + (co & 1)  # a word of the summed range behind the field, paired as the sum pairs
    assert cs + k + 2 <= len(pk["data"])
    return cs + k


def steer_zero(pk, segments=(0,)):
    """The read with the first 16-bit payload word of each chosen segment (a plain packet: a word of
    its summed range) set so that the segment's computed L4 checksum is zero: the word is the
    checksum the oracle gives the segment with that word zeroed."""
    data = bytearray(pk["data"])
    hl = hdr_len_of(pk) if kind_of(pk) != "finish" else 0
    pos = [_steer_pos(pk, hl, j) for j in segments]
    for p in pos:
        data[p:p + 2] = b"\0\0"
    st, segs = read_result(dict(pk, data=bytes(data)))
    assert st == S.OK
    f = field_of(pk)
    for j, p in zip(segments, pos):
        assert len(segs[j]) >= (hl if hl else p) + 2, "the segment has no payload word"
        data[p:p + 2] = segs[j][f:f + 2]
    return dict(pk, data=bytes(data))


def steer_ipck_zero(pk, j):
    """The IPv4 read with the first word of its source address set so that segment j's header
    checksum is 0x0000."""
    data = bytearray(pk["data"])
    data[12:14] = b"\0\0"
    st, segs = read_result(dict(pk, data=bytes(data)))
    assert st == S.OK
    data[12:14] = segs[j][10:12]
    return dict(pk, data=bytes(data))


def computed_l4(pk, seg):
    """The segment's L4 checksum recomputed bytewise from the segment itself with the field zeroed,
    before the UDP zero rule (RFC 768 / RFC 9293 / virtio NEEDS_CSUM)."""
    cs, f, k = pk["csum_start"], field_of(pk), kind_of(pk)
    b = bytearray(seg[cs:])
    b[f - cs:f - cs + 2] = b"\0\0"
    s = sum(x << 8 if i % 2 == 0 else x for i, x in enumerate(b))
    if k == "finish":
        s += (pk["data"][f] << 8) | pk["data"][f + 1]
    else:
        addrs = seg[12:20] if seg[0] >> 4 == 4 else seg[8:40]
        s += sum(x << 8 if i % 2 == 0 else x for i, x in enumerate(addrs)) + (6 if k == "tcp" else 17) + len(b)
    return ~_fold(s) & 0xFFFF


# ---- the seal_cs predicate of tx.hip, per segment ---------------------------------------------

CLAUSES = ("not_pass", "prefix_in_12_bits", "field_not_at_15", "pairs_like_start", "field_in_prefix", "under_16k",
           "power_fits")


def seal_clauses(pk, seg):
    """tx_segment_kernel's seal_cs, clause by clause, for one live segment under a single key."""
    k, cs, seg_len = kind_of(pk), pk["csum_start"], len(seg)
    gso = k in ("tcp", "udp")
    fld = field_of(pk)
    hdr_b = len(seg) - _pay_len(pk, seg) if gso else fld + 2 if k == "finish" else 0
    return dict(not_pass=k != "pass", prefix_in_12_bits=hdr_b <= 0xFFF, field_not_at_15=(fld & 15) != 15, pairs_like_start=((hdr_b - cs) & 1) == 0,
                field_in_prefix=fld + 2 <= hdr_b, under_16k=seg_len < 16384, power_fits=seal_power(pk, seg) < 1024), hdr_b


def seal_power(pk, seg):
    """e of gcm_csum_fix: the tag moves by Δ·H^e, e = payload blocks + 1 - the field block's index."""
    return ((len(seg) + 15) >> 4) + 1 - (field_of(pk) >> 4)


def _pay_len(pk, seg):
    return len(seg) - hdr_len_of(pk)


# ---- the cases --------------------------------------------------------------------------------

def _geometry(make, seed):
    """pay 0, < gso, == gso, k gso, k gso + 1 (a one-byte last segment), k gso - 1; gso odd and even."""
    out = []
    for gso, k in ((333, 3), (500, 2)):
        for pay in (0, gso - 7, gso, k * gso, k * gso + 1, k * gso - 1):
            out.append(make(rand_bytes(pay, seed + len(out)), gso))
    return out


def _refusals():
    good = lambda i: tso(4, rand_bytes(700 + i, 900 + i), 300)  # noqa: E731
    t4, t6, u4 = tso(4, rand_bytes(900, 1), 400), tso(6, rand_bytes(900, 2), 400), uso(4, rand_bytes(900, 3), 400)

    def patched(pk, off, val, **kw):
        d = bytearray(pk["data"])
        d[off] = val
        return dict(pk, data=bytes(d), **kw)

    bad = [
        tso(6, rand_bytes(500, 4), 200, ext=24, tcp_opts=40),          # hl 124: cs 64 + TCP 60
        dict(tso(4, rand_bytes(500, 5), 200, ip_opts=4), csum_start=20),  # IHL 24 > cs 20
        patched(t4, 0, 0x44),                                          # IHL 16
        patched(t4, 32, 0x40),                                         # TCP offset 16
        dict(u4, csum_start=0),                                        # cs 0 with GSO
        dict(u4, data=u4["data"][:30], csum_offset=10),                # cs + co + 1 >= len, nothing else wrong
        dict(t4, flags=S.F_NEEDS_CSUM | S.F_RSC_INFO),                 # RSC_INFO
        dict(u4, gso_type=S.GSO_UDP_L4 | S.GSO_ECN),                   # ECN on UDP_L4
        dict(u4, data=u4["data"][:19]),                                # v4 len 19
        dict(t6, data=t6["data"][:39]),                                # v6 len 39
        patched(u4, 0, 0x55),                                          # IP version 5
        dict(t4, gso_size=0),                                          # gso_size 0
        dict(t4, gso_type=S.GSO_UDP),                                  # an unknown GSO type
    ]
    out = [good(0)]
    for i, b in enumerate(bad):
        out += [b, good(i + 1)]
    return out


def cases():
    """name -> reads, in batch order. The seal-side checksum's own cases come first, so that a seal
    grid capped to one workgroup still takes them in its full passes."""
    C = {}
    R = rand_bytes
    # segment lengths 16383 / 16384 and the highest powers of H the seal multiplies by
    C["seg_len_edge"] = [
        tso(4, R(16343, 10), 20000),                   # 16383: e = 1023, every table of H^(2^j)
        tso(4, R(16344, 11), 20000),                   # 16384: summed by the segment kernel
        uso(4, R(2 * 16355, 12), 16355),               # 16383 twice, field in block 1: e = 1024
        uso(6, R(16335 + 9, 13), 16335),               # 16383 and a short one, field in block 2
        tso(6, R(16000, 14), 16000, tcp_opts=12),
    ]
    C["finish_len_edge"] = [
        finish_l4(4, 17, R(16383 - 28, 20)),           # len 16383, field in block 1: e = 1024
        finish_raw(R(16383, 21), 0, 6),                # field in block 0: e = 1025
        finish_l4(6, 6, R(16383 - 60, 22)),            # cs 40 co 16: e = 1022
        finish_l4(4, 6, R(16384 - 40, 23)),            # len 16384
    ]
    # the prefix a plain packet's seal descriptor can name is 12 bits long; past it the packet is copied whole
    C["finish_long_prefix"] = [finish_raw(R(4200, 24), 4087, 6), finish_raw(R(4300, 25), 4088, 6),
                               finish_raw(R(9000, 26), 5000, 16)]
    for name, mk in (("zero_udp4", lambda p, g: uso(4, p, g)), ("zero_udp6", lambda p, g: uso(6, p, g)),
                     ("zero_tcp4", lambda p, g: tso(4, p, g)), ("zero_tcp6", lambda p, g: tso(6, p, g, tcp_opts=12))):
        C[name] = [steer_zero(mk(R(3 * 333 + 57, 30 + len(C)), 333), (0, 1, 3))]  # first, middle, short last
    C["zero_finish"] = [steer_zero(finish_l4(4, 17, R(301, 40))), steer_zero(finish_l4(6, 6, R(77, 41))),
                        steer_zero(finish_l4(6, 17, R(2, 42)))]
    C["zero_ip_header"] = [steer_ipck_zero(tso(4, R(1000, 43), 400, ip_opts=4), 1),
                           steer_ipck_zero(uso(4, R(10, 44), 400), 0)]
    # every residue of hdr_b and of the field offset among the segments the seal sums
    C["finish_residues"] = [finish_raw(R(90 + 7 * r, 50 + r), 20 + r, 6) for r in range(16)]
    C["hdr_b_residue_1"] = [tso(4, R(700, 70), 300, gap=9)]  # hl 49: only TCP puts an eligible field there
    C["equal_run"] = [uso(6, R(48 * 64, 71), 64)]            # 48 equal segments: whole waves of one length
    C["mixed_run"] = [finish_l4(4, 17 if i % 2 else 6, R(20 + 97 * i % 1400, 72 + i)) for i in range(20)]
    C["seal_clauses"] = [plain(R(n, 80 + n)) for n in (1, 20, 777)] + [finish_raw(R(120, 84), 20, 7)]
    # header forms
    C["ip_options"] = [tso(4, R(1200, 100), 500, ip_opts=4), tso(4, R(1200, 101), 500, ip_opts=40, tcp_opts=40),
                       uso(4, R(1200, 102), 500, ip_opts=40), uso(4, R(900, 103), 500, ip_opts=4)]
    C["tcp_options"] = [tso(v, R(1100 + o, 110 + o + v), 450, tcp_opts=o) for v in (4, 6) for o in (0, 12, 40)]
    C["odd_csum_start"] = [tso(4, R(1000, 120), 333, gap=1), uso(4, R(1000, 121), 333, gap=1),
                           tso(6, R(1000, 122), 400, gap=3), uso(4, R(800, 123), 300, ip_opts=4, gap=2)]
    C["v6_extension"] = [tso(6, R(1000, 124), 400, ext=8), uso(6, R(1000, 125), 400, ext=8)]
    # wraps
    C["ipv4_id_wrap"] = [tso(4, R(2000, 130), 500, ident=0xFFFE), uso(4, R(1500, 131), 500, ident=0xFFFF),
                         uso(4, R(900, 132), 500, ident=0)]
    C["seq_wrap"] = [tso(4, R(5000, 133), 1000, seq=0xFFFFF800), tso(6, R(5000, 134), 1000, seq=0xFFFFFFFF),
                     tso(4, R(3000, 135), 1000, seq=0x0001FC00)]
    C["flag_bytes"] = [tso(4 if (n + i) % 2 else 6, R(n * 200 - 1, 140 + 4 * n + i), 200, flags=fl, ecn=bool(fl & CWR))
                       for i, fl in enumerate(FLAG_BYTES.values()) for n in (1, 2, 3)]
    # geometry
    C["geometry_tso4"] = _geometry(lambda p, g: tso(4, p, g), 200)
    C["geometry_tso6"] = _geometry(lambda p, g: tso(6, p, g), 220)
    C["geometry_uso4"] = _geometry(lambda p, g: uso(4, p, g), 240)
    C["geometry_uso6"] = _geometry(lambda p, g: uso(6, p, g), 260)
    C["gso_1"] = [uso(4, R(21, 280), 1), tso(6, R(20, 281), 1)]
    C["tile_edge"] = [tso(4, R(n, 290 + n), 1600) for n in (1535, 1536, 1537)]  # 96 payload units +- a byte
    C["gso_65535"] = [tso(4, R(30000, 300), 65535)]
    # carries
    C["finish_ones_65535"] = [finish_raw(ones(65535), 20, 6)]
    C["fills"] = [mk(v, fill(5000), 1448) for mk in (tso, uso) for v in (4, 6) for fill in (ones, zeros)] + \
                 [finish_l4(4, 17, zeros(3000)), tso(4, ones(65535 - 40), 16000)]
    # FinishChecksum forms
    C["finish_forms"] = [finish_raw(R(61 + 16 * a + 5 * b, 310 + 4 * a + b), cs, co)
                         for a, cs in enumerate((0, 20, 21, 40)) for b, co in enumerate((0, 6, 10, 16))]
    C["finish_ends"] = [finish_raw(R(48, 330), 40, 6), finish_raw(R(47, 331), 40, 6), finish_raw(R(100, 332), 40, 6)]
    C["refusals"] = _refusals()
    return C


# Cases that reach nothing another case does not, kept for what the coverage model cannot see.
REDUNDANT = ()


# ---- what the cases reach ---------------------------------------------------------------------

def _reasons(pk):
    """Why the oracle refuses this read, from the read alone (the refusals' own conditions)."""
    d, cs, co, g = pk["data"], pk["csum_start"], pk["csum_offset"], pk["gso_type"] & ~S.GSO_ECN
    k, out = kind_of(pk), set()
    ver, ihl = d[0] >> 4, (d[0] & 15) * 4
    thl = (d[cs + 12] >> 4) * 4 if k == "tcp" and len(d) > cs + 12 else None
    if g != S.GSO_NONE:
        if pk["flags"] & S.F_RSC_INFO:
            out.add("rsc_info")
        if pk["gso_type"] & S.GSO_ECN and k == "udp":
            out.add("ecn_on_udp")
        if ver == 4 and len(d) == 19:
            out.add("v4_len_19")
        if ver == 6 and len(d) == 39:
            out.add("v6_len_39")
        if ver == 5:
            out.add("ip_version_5")
        if pk["gso_size"] == 0:
            out.add("gso_size_0")
        if k == "unknown":
            out.add("unknown_gso_type")
        if cs == 0:
            out.add("csum_start_0")
        if thl == 16:
            out.add("tcp_offset_16")
        if thl == 60 and cs == 64:
            out.add("hl_124")
        if ver == 4 and ihl == 16:
            out.add("ihl_16")
        if ver == 4 and ihl > cs > 0 and ihl >= 20:
            out.add("ihl_past_csum_start")
        if len(d) >= 20 and cs + co + 1 >= len(d):
            out.add("csum_field_past_end")
    return out


REFUSALS = ("hl_124", "ihl_past_csum_start", "ihl_16", "tcp_offset_16", "csum_start_0", "csum_field_past_end", "rsc_info",
            "ecn_on_udp", "v4_len_19", "v6_len_39", "ip_version_5", "gso_size_0", "unknown_gso_type")
L4S = ("tso4", "tso6", "uso4", "uso6")


def required():
    req = [f"ihl:{n}" for n in (20, 24, 60)]
    req += [f"tcp_offset:v{v}:{n}" for v in (4, 6) for n in (20, 32, 60)]
    req += ["hl:120", "hl<=64", "hl>64"] + [f"hl%16:{r}" for r in (0, 4, 8, 12)]
    req += ["hl%4!=0", "odd_csum_start:tso", "odd_csum_start:uso", "v6_csum_start_48"]
    req += ["id_wrap:tso", "id_wrap:uso", "id0:0", "id0:65535", "seq_wrap:v4", "seq_wrap:v6", "seq_low_carry"]
    req += [f"flags:{f}:{n}" for f in FLAG_BYTES for n in ("1", "2", "3+")]
    for k in L4S:
        req += [f"{k}:{g}" for g in ("pay=0", "pay<gso", "pay=gso", "pay=k*gso", "pay=k*gso+1", "pay=k*gso-1", "gso_odd",
                                     "gso_even", "ones", "zeros")]
    req += ["gso=1:20_segments", "one_byte_last_segment"] + [f"segment_payload:{n}" for n in (1535, 1536, 1537)]
    req += ["seg_len:16383", "seg_len:16384", "finish:ones:65535", "tso:gso_size_65535", "finish:ones", "finish:zeros"]
    req += [f"zero:{k}:{w}" for k in ("udp4", "udp6", "tcp4", "tcp6") for w in ("first", "middle", "short_last")]
    req += ["zero:finish:co6", "zero:finish:co16", "ip_checksum:0"]
    req += [f"finish:cs:{n}" for n in (0, 20, 21, 40)] + [f"finish:co:{n}" for n in (0, 6, 10, 16)]
    req += ["finish:field_ends_at_len", "finish:field_ends_past_len"] + [f"finish:field%16:{r}" for r in range(16)]
    req += ["finish:len:16383", "finish:len:16384", "finish:prefix:4095", "finish:prefix:4096", "finish:prefix>4096"]
    req += [f"clause:{c}:{tf}" for c in CLAUSES for tf in ("true", "false")]
    req += [f"eligible:hdr_b%16:{r}" for r in range(16)] + [f"eligible:field%16:{r}" for r in range(15)]
    req += ["eligible:field_in_last_block", "eligible:field_in_second_block", "eligible:e:1023"]
    req += [f"eligible:e_bit:{j}" for j in range(10)]
    req += ["eligible:equal_run_of_whole_blocks", "eligible:16_distinct_lengths"]
    req += [f"refused:{r}" for r in REFUSALS]
    return req


def conditions(cs_map):
    """The set of conditions the given cases reach (the names of required())."""
    got = set()
    for reads in cs_map.values():
        res = [read_result(p) for p in reads]
        wires = []  # (eligible, length, whole payload blocks behind the prefix) of the case's segments in wire order
        for i, (pk, (st, segs)) in enumerate(zip(reads, res)):
            k = kind_of(pk)
            cs, co, d = pk["csum_start"], pk["csum_offset"], pk["data"]
            if st != S.OK:
                if k == "finish" and cs + co + 2 == len(d) + 1:
                    got.add("finish:field_ends_past_len")
                if 0 < i < len(reads) - 1 and res[i - 1][0] == S.OK and res[i + 1][0] == S.OK:
                    got.update(f"refused:{r}" for r in _reasons(pk))
                continue
            v = d[0] >> 4
            if k in ("tcp", "udp"):
                _gso_conditions(got, pk, segs, k, v)
            elif k == "finish":
                _finish_conditions(got, pk, segs[0])
            for j, seg in enumerate(segs):
                cl, hdr_b = seal_clauses(pk, seg)
                got.update(f"clause:{c}:{'true' if t else 'false'}" for c, t in cl.items())
                ok = all(cl.values())
                wires.append((ok, len(seg), len(seg) - ((hdr_b + 15) & ~15) >= 32))
                if ok:
                    f, e, m = field_of(pk), seal_power(pk, seg), (len(seg) + 15) >> 4
                    got.update((f"eligible:hdr_b%16:{hdr_b % 16}", f"eligible:field%16:{f % 16}"))
                    got.update(f"eligible:e_bit:{b}" for b in range(10) if e >> b & 1)
                    if e == 1023:
                        got.add("eligible:e:1023")
                    if f >> 4 == m - 1:
                        got.add("eligible:field_in_last_block")
                    if f >> 4 == 1:
                        got.add("eligible:field_in_second_block")
        # 31 in a row hold 16 that one wave takes, wherever the case lands in the batch
        for a in range(len(wires) - 30):
            w = wires[a:a + 31]
            if all(ok and whole for ok, _, whole in w) and len({ln for _, ln, _ in w}) == 1:
                got.add("eligible:equal_run_of_whole_blocks")
        for a in range(len(wires) - 15):
            w = wires[a:a + 16]
            if all(ok for ok, _, _ in w) and len({ln for _, ln, _ in w}) == 16:
                got.add("eligible:16_distinct_lengths")
    return got


def _gso_conditions(got, pk, segs, k, v):
    d, cs, gso = pk["data"], pk["csum_start"], pk["gso_size"]
    hl = hdr_len_of(pk)
    pay, n = len(d) - hl, len(segs)
    key = ("tso" if k == "tcp" else "uso") + str(v)
    got.add("hl<=64" if hl <= 64 else "hl>64")
    if hl == 120:
        got.add("hl:120")
    got.add(f"hl%16:{hl % 16}" if hl % 4 == 0 else "hl%4!=0")
    if cs & 1:
        got.add("odd_csum_start:" + key[:3])
    if v == 6 and cs == 48:
        got.add("v6_csum_start_48")
    if v == 4:
        ihl, id0 = (d[0] & 15) * 4, struct.unpack_from(">H", d, 4)[0]
        got.update((f"ihl:{ihl}", f"id0:{id0}"))
        if id0 + n - 1 > 0xFFFF:
            got.add("id_wrap:" + key[:3])
        if any(s[10:12] == b"\0\0" for s in segs):
            got.add("ip_checksum:0")
    if k == "tcp":
        got.add(f"tcp_offset:v{v}:{hl - cs}")
        seq0 = struct.unpack_from(">I", d, cs + 4)[0]
        last = seq0 + (n - 1) * gso
        if last >> 32:
            got.add(f"seq_wrap:v{v}")
        elif last >> 16 != seq0 >> 16:
            got.add("seq_low_carry")
        for name, fl in FLAG_BYTES.items():
            if d[cs + 13] == fl:
                got.add(f"flags:{name}:{n if n < 3 else '3+'}")
        if gso == 65535:
            got.add("tso:gso_size_65535")
    geo = {"pay=0": pay == 0, "pay<gso": 0 < pay < gso, "pay=gso": pay == gso, "pay=k*gso": pay % gso == 0 and pay >= 2 * gso,
           "pay=k*gso+1": pay % gso == 1 and pay > 2 * gso, "pay=k*gso-1": (pay + 1) % gso == 0 and pay + 1 >= 2 * gso,
           "gso_odd": gso % 2 == 1, "gso_even": gso % 2 == 0, "ones": pay >= 4096 and d[hl:] == b"\xff" * pay,
           "zeros": pay >= 4096 and d[hl:] == bytes(pay)}
    got.update(f"{key}:{g}" for g, hit in geo.items() if hit)
    if gso == 1 and n >= 20:
        got.add("gso=1:20_segments")
    if n > 1 and len(segs[-1]) - hl == 1:
        got.add("one_byte_last_segment")
    f = field_of(pk)
    for j, seg in enumerate(segs):
        pl = len(seg) - hl
        if pl in (1535, 1536, 1537):
            got.add(f"segment_payload:{pl}")
        if len(seg) in (16383, 16384):
            got.add(f"seg_len:{len(seg)}")
        if computed_l4(pk, seg) == 0 and seg[f:f + 2] == (b"\0\0" if k == "tcp" else b"\xff\xff"):
            where = "first" if j == 0 else "short_last" if j == n - 1 and n >= 3 and pl < gso else "middle" if j < n - 1 else None
            if where:
                got.add(f"zero:{k}{v}:{where}")


def _finish_conditions(got, pk, seg):
    cs, co, d = pk["csum_start"], pk["csum_offset"], pk["data"]
    got.update((f"finish:cs:{cs}", f"finish:co:{co}", f"finish:field%16:{(cs + co) % 16}", f"finish:len:{len(d)}"))
    if cs + co + 2 == len(d):
        got.add("finish:field_ends_at_len")
    if cs + co + 2 >= 4095:
        got.add(f"finish:prefix:{cs + co + 2}" if cs + co + 2 <= 4096 else "finish:prefix>4096")
    if len(d) >= 2048 and d[-2048:] == b"\xff" * 2048:
        got.add("finish:ones")
        if len(d) == 65535 and d == b"\xff" * 65535:
            got.add("finish:ones:65535")
    if len(d) >= 2048 and d[-2048:] == bytes(2048):
        got.add("finish:zeros")
    if computed_l4(pk, seg) == 0 and co in (6, 16) and seg[cs + co:cs + co + 2] == (b"\xff\xff" if co == 6 else b"\0\0"):
        got.add(f"zero:finish:co{co}")


def uncovered(cs_map):
    got = conditions(cs_map)
    return [c for c in required() if c not in got]


# ---- the directed batch -----------------------------------------------------------------------

# One rotation of the byte skews per GPU run: read i of case k starts (5 k + 3 i + rotation) mod 16
# bytes past a 16-byte boundary, so a list of four reads sees four skews in every run and a shorter
# one over the runs.
ROTATIONS = (0, 1, 6, 11, 13)


def batch(cs_map, ntun, rotation):
    """(reads, skews): the cases concatenated, case k on tunnel k mod ntun."""
    reads, skews = [], []
    for k, rs in enumerate(cs_map.values()):
        for i, p in enumerate(rs):
            reads.append(dict(p, tunnel=k % ntun))
            skews.append((5 * k + 3 * i + rotation) % 16)
    return reads, skews


def steered(cs_map):
    """The reads whose segments carry a steered zero."""
    return [p for name in ("zero_udp4", "zero_udp6", "zero_tcp4", "zero_tcp6", "zero_finish") for p in cs_map[name]]
