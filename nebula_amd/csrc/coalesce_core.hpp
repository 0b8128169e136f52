// coalesce_core.hpp — the rules of the receive-side coalescer, shared by the host form
// (coalesce.cpp), the device form (coalesce.hip) and the sanitizer program (tests/sanitize_coalesce).
// Plain C++17; compiles with g++ alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   newPacket / parseV4 / parseV6        outside.go:320-472
//   IPv6FindUpperProtocol                iputil/packet.go:349-395
//   flowKey.parseIPAt and prologues      overlay/batch/coalesce_core.go:42-94
//   ipHeadersMatch / ipv4CanCoalesceID   coalesce_core.go:104-114, :132-138
//   parsedTCP.parseTail, commitParsed    overlay/batch/tcp_coalesce.go:103-132, :181-228
//   seed / canAppend / appendPayload     tcp_coalesce.go:263-346, udp_coalesce.go:217-279
//   flushSlot, checksum seeds            tcp_coalesce.go:367-472, udp_coalesce.go:303-330
//   headersMatch / udpHeadersMatch       tcp_coalesce.go:396-419, udp_coalesce.go:334-345
//   Offload.Write / WriteGSO             overlay/tio/tio_gso_linux.go:49-55, :280-291, :325-404
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"

#if defined(__HIPCC__)
#define NEB_CO_HD __host__ __device__
#else
#define NEB_CO_HD
#endif

namespace neb {

constexpr uint32_t kCoMaxSegs = 64;      // tcpCoalesceMaxSegs / udpCoalesceMaxSegs
constexpr uint32_t kCoBufSize = 65535;   // tcpCoalesceBufSize / udpCoalesceBufSize
constexpr uint32_t kCoNone = 0xFFFFFFFFu;
enum : uint8_t { kCoLaneTcp = 0, kCoLaneUdp = 1, kCoLanePt = 2 };
// The class of a packet in its lane (commitStaged / commitParsed / seed).
enum : uint8_t {
    kCoUnparse = 0,  // fragAny or the lane parse failed: closes every chain of the lane, verbatim
    kCoSeal = 1,     // closes its flow's chain, verbatim
    kCoAck = 2,      // pure TCP ACK: verbatim, closes nothing
    kCoData = 3,     // seeds or extends a chain
    kCoPass = 4,     // passthrough lane
};
constexpr uint8_t kCoTcpPsh = 0x08, kCoTcpAck = 0x10, kCoTcpEce = 0x40;
constexpr uint8_t kCoProtoTcp = 6, kCoProtoUdp = 17, kCoProtoIcmp = 1, kCoProtoIcmp6 = 58;

NEB_CO_HD inline uint32_t co_be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
NEB_CO_HD inline uint32_t co_be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
NEB_CO_HD inline void co_put16(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}
NEB_CO_HD inline bool co_bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t lo, uint32_t hi) {
    for (uint32_t i = lo; i < hi; i++)
        if (a[i] != b[i]) return false;
    return true;
}

// ---- newPacket: the firewall's parse (only Protocol, FragAny, IPHdrLen and the error matter) ----
struct CoFw {
    uint8_t proto;
    uint8_t frag_any;
    uint16_t ip_hdr_len;
};

// IPv6FindUpperProtocol. false: ErrIPv6CouldNotFindPayload.
NEB_CO_HD inline bool co_v6_upper(const uint8_t* d, uint32_t len, uint8_t* proto, uint32_t* offset, bool* is_frag,
                                  bool* any_frag) {
    *is_frag = *any_frag = false;
    if (len < 40) return false;
    uint8_t nh = d[6];
    uint32_t off = 40;
    for (int i = 0; i < 8; i++) {  // maxIPv6ExtHeaders
        if (nh == 0 || nh == 43 || nh == 60) {
            if (len < off + 2) return false;
            nh = d[off];
            off += ((uint32_t)d[off + 1] + 1u) << 3;
        } else if (nh == 44) {
            if (len < off + 8) return false;
            *any_frag = true;
            if (d[off + 2] != 0 || (d[off + 3] & 0xf8) != 0) {  // non-first fragment: stop here
                *proto = d[off];
                *offset = off;
                *is_frag = true;
                return true;
            }
            nh = d[off];
            off += 8;
        } else if (nh == 51) {
            if (len < off + 2) return false;
            nh = d[off];
            off += ((uint32_t)d[off + 1] + 2u) << 2;
        } else {
            if (off > len) return false;
            break;
        }
    }
    *proto = nh;
    *offset = off;
    return true;
}

// newPacket(data, incoming, fp). false: the packet is dropped before Commit.
NEB_CO_HD inline bool co_new_packet(const uint8_t* d, uint32_t len, CoFw* fw) {
    fw->proto = 0;
    fw->frag_any = 0;
    fw->ip_hdr_len = 0;
    if (len < 1) return false;
    const uint32_t ver = d[0] >> 4;
    if (ver == 4) {
        if (len < 20) return false;
        const uint32_t ihl = (uint32_t)(d[0] & 0x0f) << 2;
        if (ihl < 20) return false;
        const uint32_t ff = co_be16(d + 6);
        const bool fragment = (ff & 0x1FFF) != 0;
        fw->frag_any = (ff & 0x3fff) != 0;
        fw->ip_hdr_len = (uint16_t)ihl;
        fw->proto = d[9];
        uint32_t min_len = ihl;
        if (!fragment) min_len += fw->proto == kCoProtoIcmp ? 6u : 4u;  // minFwPacketLen (+2 for ICMP)
        return len >= min_len;
    }
    if (ver == 6) {
        uint8_t proto = 0;
        uint32_t off = 0;
        bool is_frag = false, any_frag = false;
        if (!co_v6_upper(d, len, &proto, &off, &is_frag, &any_frag)) return false;
        fw->proto = proto;
        fw->frag_any = any_frag;
        fw->ip_hdr_len = (uint16_t)off;
        if (is_frag) return true;
        if (proto == kCoProtoIcmp6) {
            if (len < off + 4) return false;
            if ((d[off] == 128 || d[off] == 129) && len < off + 6) return false;  // echo request / reply
        } else if (proto == kCoProtoTcp || proto == kCoProtoUdp) {
            if (len < off + 4) return false;
        }
        return true;
    }
    return false;
}

// ---- the lane parse ----------------------------------------------------------------------------
struct CoInfo {
    uint32_t pay_len;
    uint32_t seq;
    uint16_t hdr_len;
    uint16_t ip_hdr_len;
    uint16_t ip_id;
    uint8_t v6;
    uint8_t flags;  // TCP flags byte (0 for UDP)
    uint8_t df;     // IPv4 DF
};

// flowKey.parseIPAt: the trimmed length (the IP-declared length) or 0.
NEB_CO_HD inline uint32_t co_parse_ip_at(const uint8_t* p, uint32_t len, uint32_t ip_hdr_len, CoInfo* o) {
    if (len < 20) return 0;
    const uint32_t ver = p[0] >> 4;
    if (ver == 4) {
        if (ip_hdr_len != 20) return 0;
        if (((uint32_t)(p[0] & 0x0f) << 2) != 20) return 0;
        if (co_be16(p + 6) & 0x3fff) return 0;
        const uint32_t total = co_be16(p + 2);
        if (total > len || total < 20) return 0;
        o->v6 = 0;
        o->ip_id = (uint16_t)co_be16(p + 4);
        o->df = (p[6] & 0x40) != 0;
        return total;
    }
    if (ver == 6) {
        if (ip_hdr_len != 40 || len < 40) return 0;
        const uint32_t pl = co_be16(p + 4);
        if (40 + pl > len) return 0;
        o->v6 = 1;
        o->ip_id = 0;
        o->df = 0;
        return 40 + pl;
    }
    return 0;
}

// parsedTCP.parseAt / parsedUDP.parseAt. false: the packet is unparseable for its lane.
NEB_CO_HD inline bool co_lane_parse(const uint8_t* p, uint32_t len, uint32_t ip_hdr_len, bool tcp, CoInfo* o) {
    const uint32_t t = co_parse_ip_at(p, len, ip_hdr_len, o);
    if (!t) return false;
    const uint32_t ip = ip_hdr_len;
    o->ip_hdr_len = (uint16_t)ip;
    if (tcp) {
        if (t < ip + 20) return false;
        const uint32_t off = (uint32_t)(p[ip + 12] >> 4) * 4;
        if (off < 20 || off > 60) return false;
        if (t < ip + off) return false;
        o->hdr_len = (uint16_t)(ip + off);
        o->pay_len = t - o->hdr_len;
        o->seq = co_be32(p + ip + 4);
        o->flags = p[ip + 13];
        return true;
    }
    if (t < ip + 8) return false;
    const uint32_t ulen = co_be16(p + ip + 4);
    if (ulen < 8 || ulen > t - ip) return false;
    o->hdr_len = (uint16_t)(ip + 8);
    o->pay_len = ulen - 8;
    o->seq = 0;
    o->flags = 0;
    return true;
}

// The class of a lane-parsed packet (commitParsed's admission, the zero-length rules, seed's size cap:
// a packet with hdrLen + payLen > 65535 can never append, so it always reaches seed and seals).
NEB_CO_HD inline uint8_t co_class(bool tcp, const CoInfo& o) {
    if (tcp) {
        if (!(o.flags & kCoTcpAck) || (o.flags & ~(kCoTcpAck | kCoTcpPsh | kCoTcpEce))) return kCoSeal;
        if (o.pay_len == 0) return kCoAck;
    } else if (o.pay_len == 0) {
        return kCoSeal;
    }
    if ((uint32_t)o.hdr_len + o.pay_len > kCoBufSize) return kCoSeal;
    return kCoData;
}

// The 38-byte flow key {src16, dst16, sport, dport, isV6} of a lane-parsed packet.
constexpr uint32_t kCoKeyLen = 38;
NEB_CO_HD inline void co_flow_key(const uint8_t* p, const CoInfo& o, uint8_t k[38]) {
    for (int i = 0; i < 38; i++) k[i] = 0;
    if (o.v6) {
        for (int i = 0; i < 32; i++) k[i] = p[8 + i];
    } else {
        for (int i = 0; i < 4; i++) {
            k[i] = p[12 + i];
            k[16 + i] = p[16 + i];
        }
    }
    for (int i = 0; i < 4; i++) k[32 + i] = p[o.ip_hdr_len + i];
    k[36] = 0;
    k[37] = o.v6;
}
// Key equality straight from two lane-parsed packets (no key is materialised on the device).
NEB_CO_HD inline bool co_flow_equal(const uint8_t* a, const CoInfo& ia, const uint8_t* b, const CoInfo& ib) {
    if (ia.v6 != ib.v6) return false;
    if (ia.v6 ? !co_bytes_eq(a, b, 8, 40) : !co_bytes_eq(a, b, 12, 20)) return false;
    return co_bytes_eq(a + ia.ip_hdr_len, b + ib.ip_hdr_len, 0, 4);
}
// A 32-bit hash of the key: orders and groups, never decides equality.
NEB_CO_HD inline uint32_t co_flow_hash(const uint8_t* p, const CoInfo& o) {
    uint32_t h = 0x811C9DC5u ^ o.v6;
    const uint32_t a0 = o.v6 ? 8u : 12u, a1 = o.v6 ? 40u : 20u;
    for (uint32_t i = a0; i < a1; i++) h = (h ^ p[i]) * 0x01000193u;
    for (uint32_t i = 0; i < 4; i++) h = (h ^ p[o.ip_hdr_len + i]) * 0x01000193u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

// ---- canAppend ----------------------------------------------------------------------------------
// headersMatch / udpHeadersMatch over two headers of the same length hdr_len.
NEB_CO_HD inline bool co_headers_match(const uint8_t* a, const uint8_t* b, bool v6, uint32_t ip, uint32_t hdr_len,
                                       bool tcp) {
    if (v6) {
        if (!co_bytes_eq(a, b, 0, 4) || !co_bytes_eq(a, b, 6, 40)) return false;
    } else {
        if (!co_bytes_eq(a, b, 0, 2) || !co_bytes_eq(a, b, 6, 10) || !co_bytes_eq(a, b, 12, 20)) return false;
    }
    if (!co_bytes_eq(a, b, ip, ip + 4)) return false;
    if (!tcp) return true;
    return co_bytes_eq(a, b, ip + 8, ip + 13) && co_bytes_eq(a, b, ip + 14, ip + 16) &&
           co_bytes_eq(a, b, ip + 18, hdr_len);
}

// An open chain, as the reference's coalesceSlot keeps it.
struct CoChain {
    uint32_t first;  // the seed's input index
    uint32_t nseg;
    uint32_t total_pay;
    uint32_t gso;
    uint32_t next_seq;
    uint16_t hdr_len;
    uint16_t ip_hdr_len;
    uint8_t v6;
    uint8_t psh;  // PSH seen on an appended segment
};

NEB_CO_HD inline void co_seed(CoChain* s, uint32_t first, const CoInfo& o) {
    s->first = first;
    s->nseg = 1;
    s->total_pay = o.pay_len;
    s->gso = o.pay_len;
    s->next_seq = o.seq + o.pay_len;
    s->hdr_len = o.hdr_len;
    s->ip_hdr_len = o.ip_hdr_len;
    s->v6 = o.v6;
    s->psh = 0;
}

// canAppend against the seed's (pristine) packet.
NEB_CO_HD inline bool co_can_append(const CoChain& s, const uint8_t* seed, const uint8_t* p, const CoInfo& o,
                                    bool tcp) {
    if (o.hdr_len != s.hdr_len) return false;
    if (tcp && o.seq != s.next_seq) return false;
    if (s.nseg >= kCoMaxSegs) return false;
    if (o.pay_len > s.gso) return false;
    if ((uint32_t)s.hdr_len + s.total_pay + o.pay_len > kCoBufSize) return false;
    if (tcp && ((seed[s.ip_hdr_len + 13] ^ o.flags) & kCoTcpEce)) return false;
    if (!s.v6 && !(seed[6] & 0x40) && co_be16(p + 4) != ((co_be16(seed + 4) + s.nseg) & 0xFFFF)) return false;
    return co_headers_match(seed, p, s.v6, s.ip_hdr_len, s.hdr_len, tcp);
}

// appendPayload: true when the chain is now closed.
NEB_CO_HD inline bool co_append(CoChain* s, const CoInfo& o, bool tcp) {
    s->nseg++;
    s->total_pay += o.pay_len;
    s->next_seq = o.seq + o.pay_len;
    const bool psh = tcp && (o.flags & kCoTcpPsh);
    if (psh) s->psh = 1;
    return o.pay_len < s->gso || psh;
}

// The same admission between two consecutive data packets p then q of one flow: every comparison
// canAppend makes against the seed is an equality or a +1 chain, so comparing neighbours is
// equivalent. The size rules (gso, 64 segments, 65535 bytes) are not part of it.
NEB_CO_HD inline bool co_link(const uint8_t* p, const CoInfo& ip, const uint8_t* q, const CoInfo& iq, bool tcp) {
    if (ip.hdr_len != iq.hdr_len || ip.v6 != iq.v6) return false;
    if (tcp && iq.seq != ip.seq + ip.pay_len) return false;
    if (tcp && ((ip.flags ^ iq.flags) & kCoTcpEce)) return false;
    if (!ip.v6 && !ip.df && iq.ip_id != (uint16_t)(ip.ip_id + 1)) return false;
    return co_headers_match(p, q, ip.v6, ip.ip_hdr_len, ip.hdr_len, tcp);
}

// ---- flushSlot ----------------------------------------------------------------------------------
NEB_CO_HD inline uint16_t co_fold_once_no_invert(uint32_t sum) {
    while (sum >> 16) sum = (sum & 0xffff) + (sum >> 16);
    return (uint16_t)sum;
}
NEB_CO_HD inline uint32_t co_pseudo_sum_v4(const uint8_t* src, const uint8_t* dst, uint8_t proto, uint32_t l4_len) {
    return co_be16(src) + co_be16(src + 2) + co_be16(dst) + co_be16(dst + 2) + proto + l4_len;
}
NEB_CO_HD inline uint32_t co_pseudo_sum_v6(const uint8_t* src, const uint8_t* dst, uint8_t proto, uint32_t l4_len) {
    uint32_t sum = 0;
    for (int i = 0; i < 16; i += 2) sum += co_be16(src + i) + co_be16(dst + i);
    return sum + (l4_len >> 16) + (l4_len & 0xffff) + proto;
}
NEB_CO_HD inline uint16_t co_ipv4_hdr_checksum(const uint8_t* hdr, uint32_t n) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i + 1 < n; i += 2) sum += co_be16(hdr + i);
    if (n & 1) sum += (uint32_t)hdr[n - 1] << 8;
    while (sum >> 16) sum = (sum & 0xffff) + (sum >> 16);
    return (uint16_t)~sum;
}
// Patch a copy of the seed's header (hdr_len bytes) into the superpacket's.
NEB_CO_HD inline void co_patch_header(uint8_t* hdr, bool v6, uint32_t ip, uint32_t hdr_len, uint32_t total_pay,
                                      bool tcp, bool psh) {
    const uint32_t total = hdr_len + total_pay, l4 = total - ip;
    if (v6) {
        co_put16(hdr + 4, l4);
    } else {
        co_put16(hdr + 2, total);
        hdr[10] = hdr[11] = 0;
        co_put16(hdr + 10, co_ipv4_hdr_checksum(hdr, ip));
    }
    if (!tcp) co_put16(hdr + ip + 4, l4);
    const uint8_t proto = tcp ? kCoProtoTcp : kCoProtoUdp;
    const uint32_t ps = v6 ? co_pseudo_sum_v6(hdr + 8, hdr + 24, proto, l4) : co_pseudo_sum_v4(hdr + 12, hdr + 16, proto, l4);
    co_put16(hdr + ip + (tcp ? 16 : 6), co_fold_once_no_invert(ps));
    if (tcp && psh) hdr[ip + 13] |= kCoTcpPsh;
}

// ---- the virtio header of a write ------------------------------------------------------------------
NEB_CO_HD inline void co_write_verbatim(neb_tun_write* w, uint64_t out_off, uint32_t len, uint32_t first,
                                        uint8_t lane) {
    w->out_off = out_off;
    w->len = len;
    w->first = first;
    w->nseg = 1;
    w->vnet_flags = NEB_VNET_F_DATA_VALID;
    w->gso_type = NEB_GSO_NONE;
    w->hdr_len = w->gso_size = w->csum_start = w->csum_offset = 0;
    w->lane = lane;
    w->reserved[0] = w->reserved[1] = w->reserved[2] = 0;
}
NEB_CO_HD inline void co_write_chain(neb_tun_write* w, uint64_t out_off, uint32_t first, uint32_t nseg,
                                     uint32_t hdr_len, uint32_t ip, uint32_t total_pay, uint32_t gso, bool v6,
                                     bool tcp) {
    w->out_off = out_off;
    w->len = hdr_len + total_pay;
    w->first = first;
    w->nseg = (uint16_t)nseg;
    w->vnet_flags = NEB_VNET_F_NEEDS_CSUM;
    w->gso_type = tcp ? (v6 ? NEB_GSO_TCPV6 : NEB_GSO_TCPV4) : NEB_GSO_UDP_L4;
    w->hdr_len = (uint16_t)hdr_len;
    w->gso_size = (uint16_t)gso;
    w->csum_start = (uint16_t)ip;
    w->csum_offset = tcp ? 16 : 6;
    w->lane = tcp ? kCoLaneTcp : kCoLaneUdp;
    w->reserved[0] = w->reserved[1] = w->reserved[2] = 0;
}
NEB_CO_HD inline uint64_t co_align16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// The lane of a committed packet.
NEB_CO_HD inline uint8_t co_lane(uint8_t proto, uint32_t lanes) {
    if (proto == kCoProtoTcp && (lanes & NEB_COALESCE_TCP)) return kCoLaneTcp;
    if (proto == kCoProtoUdp && (lanes & NEB_COALESCE_UDP)) return kCoLaneUdp;
    return kCoLanePt;
}

// One packet, fully classified: what both forms compute first.
struct CoRec {
    CoInfo info;
    uint8_t lane;
    uint8_t cls;
    int32_t status;  // NEB_STATUS_OK, NEB_STATUS_INVALID (dropped), NEB_STATUS_NOT_MESSAGE (skipped)
};
NEB_CO_HD inline void co_classify(const neb_plain_packet& pp, const uint8_t* p, uint32_t lanes, CoRec* r) {
    r->info = CoInfo{};
    r->lane = kCoLanePt;
    r->cls = kCoPass;
    r->status = NEB_STATUS_OK;
    if (pp.flags & NEB_PLAIN_SKIP) {
        r->status = NEB_STATUS_NOT_MESSAGE;
        return;
    }
    CoFw fw;
    if (pp.flags & NEB_PLAIN_PARSED) {
        fw.proto = pp.proto;
        fw.frag_any = (pp.flags & NEB_PLAIN_FRAG_ANY) != 0;
        fw.ip_hdr_len = pp.ip_hdr_len;
        if (pp.len == 0) {  // Offload.Write of an empty buffer writes nothing
            r->status = NEB_STATUS_INVALID;
            return;
        }
    } else if (!co_new_packet(p, pp.len, &fw)) {
        r->status = NEB_STATUS_INVALID;
        return;
    }
    r->lane = co_lane(fw.proto, lanes);
    if (r->lane == kCoLanePt) return;
    const bool tcp = r->lane == kCoLaneTcp;
    if (fw.frag_any || !co_lane_parse(p, pp.len, fw.ip_hdr_len, tcp, &r->info)) {
        r->cls = kCoUnparse;
        return;
    }
    r->cls = co_class(tcp, r->info);
}

// neb_rx_plain_from_wire for one packet.
NEB_CO_HD inline void co_plain_from_wire(const neb_rx_packet& pk, int32_t status, const uint8_t* arena,
                                         const uint64_t* epoch, uint32_t nepoch, neb_plain_packet* o) {
    const uint32_t len = pk.len & ~NEB_RX_OWN_SOURCE;
    o->off = 0;
    o->epoch = 0;
    o->counter = 0;
    o->len = 0;
    o->ip_hdr_len = 0;
    o->proto = 0;
    o->flags = NEB_PLAIN_SKIP;
    if (status != NEB_STATUS_OK || len < 32 || pk.key_id >= nepoch) return;
    const uint8_t* h = arena + pk.off;
    if ((h[0] & 0x0f) != 1 || h[1] != 0) return;  // header type Message, subtype None (outside.go:145-149)
    o->off = pk.off + 16;
    o->len = len - 32;
    o->counter = ((uint64_t)co_be32(h + 8) << 32) | co_be32(h + 12);
    o->epoch = epoch[pk.key_id];
    o->flags = 0;
}

}  // namespace neb
