"""TEST INFRASTRUCTURE ONLY: the inputs of tests/test_rx_coalesce.py and tests/test_gpu_rx_coalesce.py —
one named batch per scenario of the reference's tcp_coalesce_test.go, udp_coalesce_test.go and
multi_coalesce_test.go (rebuilt from what each test describes), a randomised mix, a well-formed bulk
batch for the round trip through the segmentation oracle, and the comparison with the model
(coalesce_ref.py)."""
import random

import numpy as np

import coalesce_ref as M
from nebula_amd import _lib as L

A, B, C2 = M.ip4("10.0.0.1"), M.ip4("10.0.0.2"), M.ip4("10.0.0.3")
A6, B6 = M.ip6(1), M.ip6(2)
BOTH = M.COALESCE_TCP | M.COALESCE_UDP


def P(data, counter, epoch=0, **kw):
    return dict(data=data, epoch=epoch, counter=counter, **kw)


def pay(n, tag=0):
    return bytes((tag + 7 * i) & 0xFF for i in range(n))


def seg(i, size=1200, flags=M.ACK, sport=1000, src=A, dst=B, seq0=1000, n=None, **kw):
    """Segment i of a v4 flow: seq advances by `size`, the IPv4 ID by one."""
    kw.setdefault("ident", 100 + i)
    return M.tcp4(src, dst, sport, 80, seq0 + i * size, pay(size if n is None else n, i), flags, **kw)


def seg6(i, size=1200, flags=M.ACK, sport=1000, n=None, **kw):
    return M.tcp6(A6, B6, sport, 80, 1000 + i * size, pay(size if n is None else n, i), flags, **kw)


def dgram(i, size=1000, sport=2000, n=None, **kw):
    kw.setdefault("ident", 300 + i)
    return M.udp4(A, B, sport, 53, pay(size if n is None else n, i), **kw)


def seq_(pkts, **kw):
    return [P(d, c + 1, **kw) for c, d in enumerate(pkts)]


def v6_frag_first(inner_proto, l4):
    return M.ipv6(A6, B6, 44, bytes([inner_proto, 0, 0, 1]) + b"\0\0\0\7" + l4)


def named_cases():
    """[(name, packets, lanes)]"""
    c = []
    add = lambda name, pk, lanes=BOTH: c.append((name, pk, lanes))  # noqa: E731
    # ---- tcp_coalesce_test.go
    add("tcp_seed_then_flush_alone", seq_([seg(0)]))
    add("tcp_pure_ack_does_not_seal", seq_([seg(0), seg(1, n=0), seg(1), seg(2)]))
    for nm, fl in (("fin", M.FIN | M.ACK), ("syn", M.SYN), ("cwr", M.CWR | M.ACK), ("rst", M.RST | M.ACK)):
        add(f"tcp_{nm}_seals_flow", seq_([seg(0), seg(1), seg(2, flags=fl), seg(3), seg(4)]))
    add("tcp_adjacent_coalesce", seq_([seg(i) for i in range(4)]))
    add("tcp_seq_gap", seq_([seg(0), seg(1), seg(3), seg(4)]))
    add("tcp_ece_mismatch", seq_([seg(0), seg(1, flags=M.ACK | M.ECE), seg(2, flags=M.ACK | M.ECE), seg(3)]))
    add("tcp_urg_flag", seq_([seg(0), seg(1, flags=M.ACK | M.URG), seg(2)]))
    add("tcp_ect0_vs_ect1", seq_([seg(0, tos=2), seg(1, tos=1), seg(2, tos=1)]))
    add("tcp_dscp_mismatch", seq_([seg(0, tos=0x20), seg(1), seg(2)]))
    add("tcp_window_mismatch", seq_([seg(0), seg(1, tcp_kw=dict(window=500)), seg(2, tcp_kw=dict(window=500))]))
    add("tcp_short_last_closes",
        seq_([seg(0), seg(1), seg(2, n=500), M.tcp4(A, B, 1000, 80, 1000 + 2900, pay(1200), ident=103),
              M.tcp4(A, B, 1000, 80, 1000 + 4100, pay(1200), ident=104)]))
    add("tcp_psh_finalises_and_propagates", seq_([seg(0), seg(1), seg(2, flags=M.ACK | M.PSH), seg(3), seg(4)]))
    add("tcp_psh_on_seed", seq_([seg(0, flags=M.ACK | M.PSH), seg(1), seg(2)]))
    add("tcp_different_flow", seq_([seg(0), seg(0, sport=1001), seg(0, src=C2)]))
    add("tcp_ip_options", seq_([seg(0), seg(1), seg(2, options=b"\1\1\1\1"), seg(3), seg(4)]))
    add("tcp_options_timestamps", seq_([seg(i, tcp_kw=dict(options=b"\1\1\x08\x0a" + bytes(8))) for i in range(3)]
                                       + [seg(3, tcp_kw=dict(options=b"\1\1\x08\x0a" + bytes(7) + b"\1"))]))
    add("tcp_cap_64_segments", seq_([seg(i, size=100) for i in range(70)]))
    add("tcp_cap_65535_bytes", seq_([seg(i, size=1300) for i in range(60)]))
    add("tcp_larger_than_seed", seq_([seg(0, n=500), M.tcp4(A, B, 1000, 80, 1500, pay(900), ident=101)]))
    inter = []
    for i in range(4):
        inter += [seg(i), seg(i, sport=1001), seg(i, sport=1002, src=C2)]
    add("tcp_interleaved_flows_creation_order", seq_(inter))
    add("tcp_v6_ece_flow", seq_([seg6(i, flags=M.ACK | M.ECE) for i in range(3)]))
    add("tcp_v6_differing_ecn", seq_([seg6(0, tc=2), seg6(1, tc=1), seg6(2, tc=1)]))
    add("tcp_v6_flow_label", seq_([seg6(0, flow=5), seg6(1, flow=5), seg6(2, flow=6)]))
    add("tcp_df_clear_sequential_ids", seq_([seg(i, df=False) for i in range(4)]))
    add("tcp_df_clear_id_gap", seq_([seg(0, df=False), seg(1, df=False), seg(2, df=False, ident=110),
                                     seg(3, df=False, ident=111)]))
    add("tcp_df_clear_id_wrap", seq_([seg(i, df=False, ident=(0xFFFE + i) & 0xFFFF) for i in range(4)]))
    add("tcp_df_set_random_ids", seq_([seg(i, ident=(7919 * (i + 3)) & 0xFFFF) for i in range(4)]))
    add("tcp_seq_wraparound", seq_([seg(i, seq0=0xFFFFFFFF - 600) for i in range(3)]))
    add("tcp_unparseable_seals_all",
        seq_([seg(0), seg(0, sport=1001), seg(1, mf=True), seg(1), seg(1, sport=1001), seg(2), seg(2, sport=1001)]))
    add("tcp_trailing_bytes_trimmed", seq_([seg(0) + b"\xEE" * 5, seg(1) + b"\xDD" * 3, seg(2)]))
    add("tcp_total_length_beyond_packet", seq_([seg(0), seg(1)[:-10], seg(2)]))
    # ---- udp_coalesce_test.go
    add("udp_equal_sized", seq_([dgram(i) for i in range(4)]))
    add("udp_short_last", seq_([dgram(0), dgram(1), dgram(2, n=300), dgram(3), dgram(4)]))
    add("udp_larger_than_seed_reseeds", seq_([dgram(0, n=500), dgram(1, n=800), dgram(2, n=800)]))
    add("udp_max_segments", seq_([dgram(i, size=100) for i in range(70)]))
    add("udp_cap_65535_bytes", seq_([dgram(i, size=1400) for i in range(50)]))
    add("udp_zero_length_seals_keeps_order", seq_([dgram(0), dgram(1), dgram(2, n=0), dgram(3), dgram(4)]))
    add("udp_v4_fragment_and_options",
        seq_([dgram(0), dgram(1), dgram(2, mf=True), dgram(3), dgram(4, options=b"\1\1\1\1"), dgram(5), dgram(6)]))
    add("udp_v6", seq_([M.udp6(A6, B6, 2000, 53, pay(900, i)) for i in range(3)]))
    add("udp_different_ports", seq_([dgram(0), dgram(1, sport=2001), dgram(2)]))
    bad = bytearray(dgram(1))
    bad[24:26] = (4).to_bytes(2, "big")  # UDP length < 8
    add("udp_bad_length", seq_([dgram(0), bytes(bad), dgram(2)]))
    # ---- multi_coalesce_test.go
    mix = [seg(0), dgram(0), M.icmp4(A, B, 7, pay(40)), seg(1), dgram(1), M.icmp6(A6, B6, 9, pay(30)), seg(2),
           dgram(2), M.ipv4(A, B, 47, pay(64))]
    add("multi_routes_by_proto", seq_(mix))
    order = [5, 0, 3, 1, 2, 4, 8, 6, 7, 10, 9, 11]
    flows = []
    for i in range(4):
        flows += [seg(i), seg(i, sport=1001), dgram(i)]
    add("multi_restores_transmission_order", [P(flows[j], j + 1) for j in order])
    add("multi_epoch_orders_across_rehandshake",
        [P(seg(3), 1, epoch=2), P(seg(4), 2, epoch=2), P(seg(0), 100, epoch=1), P(seg(1), 101, epoch=1),
         P(seg(2), 102, epoch=1), P(seg(5), 3, epoch=2)])
    add("multi_lanes_without_udp", [P(flows[j], j + 1) for j in order], M.COALESCE_TCP)
    add("multi_lanes_without_tcp", [P(flows[j], j + 1) for j in order], M.COALESCE_UDP)
    add("multi_lanes_none_still_sorts", [P(flows[j], j + 1) for j in order], 0)
    l4 = M.tcp_hdr(A6, B6, 1000, 80, 1000 + 2400, pay(600))
    add("multi_v6_fragment_stays_in_lane",
        seq_([seg6(0), seg6(1), v6_frag_first(M.TCP, l4), seg6(2), seg6(3), M.udp6(A6, B6, 2000, 53, pay(500)),
              v6_frag_first(M.UDP, M.udp_hdr(A6, B6, 2000, 53, pay(500))), M.udp6(A6, B6, 2000, 53, pay(500))]))
    # ---- the record's own fields
    pk = seq_([seg(0), seg(1), seg(2), dgram(0), dgram(1)])
    pk[1]["flags"] = M.PLAIN_SKIP
    add("record_skip", pk)
    pk = seq_([seg(0), seg(1), b"\x45", b"", b"\x60" + bytes(20), seg(2), dgram(0)])
    add("record_derived_parse_drops", pk)
    pk = seq_([seg(0), seg(1), seg(2), dgram(0), dgram(1)])
    for p in pk[:3]:
        p.update(flags=M.PLAIN_PARSED, proto=M.TCP, ip_hdr_len=20)
    pk[2]["flags"] |= M.PLAIN_FRAG_ANY
    pk[3].update(flags=M.PLAIN_PARSED, proto=M.UDP, ip_hdr_len=24)  # a wrong offset: unparseable in its lane
    pk[4].update(flags=M.PLAIN_PARSED, proto=M.ICMP, ip_hdr_len=20)  # the caller's protocol routes
    add("record_caller_parse", pk)
    return c


# ---- randomised mix --------------------------------------------------------------------------------
def random_batch(seed, n):
    """9 tunnels, about 40 flows of TCP / UDP / ICMP over v4 / v6, bursts, about 5% of the packets
    reordered inside windows of 8, and every irregularity the lanes react to."""
    r = random.Random(seed)
    flows = []
    for f in range(40):
        kind = r.choice(["tcp4", "tcp4", "tcp4", "tcp6", "tcp6", "udp4", "udp4", "udp6", "icmp4", "icmp6"])
        flows.append(dict(kind=kind, tun=r.randrange(9), sport=1000 + f, seq=r.randrange(1 << 32), id=r.randrange(65536),
                          df=r.random() < 0.6, size=r.choice([100, 536, 1200, 1300, 1400]), ece=False,
                          src=M.ip4(f"10.1.{f % 7}.{1 + f % 3}"), src6=M.ip6(100 + f % 5)))
    ctr = [r.randrange(1, 1000) for _ in range(9)]
    out = []
    while len(out) < n:
        fl = r.choice(flows)
        for _ in range(r.randrange(1, 24)):
            if len(out) >= n:
                break
            t = fl["tun"]
            ctr[t] += 1
            k, size, x = fl["kind"], fl["size"], r.random()
            flags, ln, ipkw, fk = M.ACK, size, {}, 0
            if x < 0.02:
                flags = M.ACK | M.FIN
            elif x < 0.06:
                flags = M.ACK | M.PSH
            elif x < 0.10:
                ln = 0
            elif x < 0.12:
                fl["seq"] += 7
            elif x < 0.14:
                fl["id"] += 3
            elif x < 0.16:
                fl["ece"] = not fl["ece"]
            elif x < 0.18:
                ipkw = dict(mf=True)
            elif x < 0.20:
                ipkw = dict(options=b"\1\1\1\1")
            elif x < 0.26:
                ln = r.randrange(1, size)
            elif x < 0.27:
                ln = size + 8
            if fl["ece"]:
                flags |= M.ECE
            body = pay(ln, len(out))
            if k[-1] == "6":
                ipkw = {}
            else:
                ipkw.update(ident=fl["id"] & 0xFFFF, df=fl["df"])
                fl["id"] += 1
            if k == "tcp4":
                d = M.tcp4(fl["src"], B, fl["sport"], 80, fl["seq"], body, flags, **ipkw)
            elif k == "tcp6":
                d = M.tcp6(fl["src6"], B6, fl["sport"], 80, fl["seq"], body, flags)
            elif k == "udp4":
                d = M.udp4(fl["src"], B, fl["sport"], 53, body, **ipkw)
            elif k == "udp6":
                d = M.udp6(fl["src6"], B6, fl["sport"], 53, body)
            elif k == "icmp4":
                d = M.icmp4(fl["src"], B, fl["sport"], body, **ipkw)
            else:
                d = M.icmp6(fl["src6"], B6, fl["sport"], body)
            if k.startswith("tcp"):
                fl["seq"] = (fl["seq"] + ln) & 0xFFFFFFFF
            y = r.random()
            if y < 0.01:
                d = d[:r.randrange(0, 24)]  # a runt for the derived parse
            elif y < 0.02:
                fk = M.PLAIN_SKIP
            p = P(d, ctr[t], epoch=10 + t, flags=fk)
            if not fk and y > 0.7:
                pp = M.new_packet(d)
                if pp is not None:  # the caller's firewall parse instead of the derived one
                    p.update(flags=M.PLAIN_PARSED | (M.PLAIN_FRAG_ANY if pp[1] else 0), proto=pp[0], ip_hdr_len=pp[2])
            out.append(p)
    for b in range(0, n - 8, 8):  # reorder inside windows of 8
        if r.random() < 0.2:
            i, j = r.sample(range(b, b + 8), 2)
            out[i], out[j] = out[j], out[i]
    return out


# ---- the well-formed bulk batch of the round trip -------------------------------------------------------
def bulk_batch(seed, nflows=12, runs=6):
    """TCP (sequential IPv4 IDs, PSH only on a run's last packet) and UDP flows over v4 and v6, with
    valid checksums and no trailing bytes: every chain must segment back into its packets."""
    r = random.Random(seed)
    out, ctr = [], 0
    for f in range(nflows):
        kind = ["tcp4", "tcp6", "udp4", "udp6"][f % 4]
        seq, ident, df = r.randrange(1 << 32), r.randrange(65536), f % 8 < 4
        for _ in range(runs):
            size = r.choice([100, 536, 1300, 1448])
            cnt = r.randrange(1, 80)
            for i in range(cnt):
                last = i == cnt - 1
                ln = r.randrange(1, size + 1) if last else size
                body = bytes(r.getrandbits(8) for _ in range(ln))
                fl = M.ACK | (M.PSH if last else 0)
                kw = dict(ident=ident & 0xFFFF, df=df)
                if kind == "tcp4":
                    d = M.tcp4(A, B, 1000 + f, 80, seq, body, fl, **kw)
                elif kind == "tcp6":
                    d = M.tcp6(A6, B6, 1000 + f, 80, seq, body, fl)
                elif kind == "udp4":
                    d = M.udp4(A, B, 2000 + f, 53, body, **kw)
                else:
                    d = M.udp6(A6, B6, 2000 + f, 53, body)
                seq = (seq + ln) & 0xFFFFFFFF
                ident += 1
                ctr += 1
                out.append(P(d, ctr))
    return out


# ---- running a batch and comparing with the model -------------------------------------------------------
def stage(packets):
    """-> (plain records, input arena): packets back to back, so offsets fall at every alignment."""
    plain = np.zeros(len(packets), L.PLAIN_PACKET_DTYPE)
    parts, off = [], 3
    for i, p in enumerate(packets):
        d = p["data"]
        plain[i] = (off, p["epoch"], p["counter"], len(d), p.get("ip_hdr_len", 0), p.get("proto", 0), p.get("flags", 0))
        parts.append(d)
        off += len(d)
    return plain, np.frombuffer(b"\xA5" * 3 + b"".join(parts) + b"\x5A" * 16, np.uint8).copy()


STAGE_LEAD = 3  # the filler in front of the first record, as in stage


def stage_padded(packets, pads=None):
    """stage with pads[i] filler bytes in front of record i (default: the packet's own "pad", or
    none), so a record's source offset can fall at a chosen residue mod 16. Without pads: stage."""
    if pads is None:
        pads = [p.get("pad", 0) for p in packets]
    plain = np.zeros(len(packets), L.PLAIN_PACKET_DTYPE)
    parts, off = [b"\xA5" * STAGE_LEAD], STAGE_LEAD
    for i, (p, pad) in enumerate(zip(packets, pads)):
        d = p["data"]
        off += pad
        plain[i] = (off, p["epoch"], p["counter"], len(d), p.get("ip_hdr_len", 0), p.get("proto", 0), p.get("flags", 0))
        parts += [b"\x3C" * pad, d]
        off += len(d)
    return plain, np.frombuffer(b"".join(parts) + b"\x5A" * 16, np.uint8).copy()


def default_cap(packets):
    return sum(M.align16(len(p["data"])) for p in packets)


FIELDS = ("out_off", "len", "first", "nseg", "vnet_flags", "gso_type", "hdr_len", "gso_size", "csum_start",
          "csum_offset", "lane")


def assert_equal_model(model, got, what=""):
    """model: coalesce_ref.coalesce(...); got: (writes, out, pkt_write, pkt_status) of a form."""
    mw, mpw, mst = model
    writes, out, pw, ps = got
    assert len(writes) == len(mw), f"{what}: nwrites {len(writes)} != {len(mw)}"
    assert [int(x) for x in ps] == mst, f"{what}: pkt_status"
    assert [int(x) & 0xFFFFFFFF for x in pw] == mpw, f"{what}: pkt_write"
    for k, (w, m) in enumerate(zip(writes, mw)):
        for f in FIELDS:
            assert int(w[f]) == m[f], f"{what}: write {k} {f}: {int(w[f])} != {m[f]}"
        assert not w["reserved"].any()
        o = int(w["out_off"])
        assert out[o:o + m["len"]].tobytes() == m["data"], f"{what}: write {k} bytes"
