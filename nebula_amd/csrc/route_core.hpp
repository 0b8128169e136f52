// route_core.hpp — the rules of the TX resolve (neb_tx_table_*, neb_tx_resolve_batch), shared by the
// host table and host form (route.cpp), the device form (route.hip) and the sanitizer program
// (tests/sanitize_route). Plain C++17; compiles with g++ alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   newPacket / parseV4 / parseV6          outside.go:320-472 (incoming == false; == true for peer_core.hpp)
//   IPv6FindUpperProtocol                  iputil/packet.go:349-395
//   the broadcast, self, multicast gates   inside.go:43-76, pki.go:475-487
//   getOrHandshakeConsiderRouting          inside.go:292-372
//   RoutesFor (longest prefix)             overlay/tun_linux.go:366-369
//   hashPacket / BalancePacket             routing/balance.go:14-39
//   CalculateBucketsForGateways            routing/gateway.go:48-70
//   netip.Prefix.Contains                  a v4 address only in v4 prefixes, 4-in-6 only in v6 ones
//   [ext] netip.Addr.IsMulticast           Go's stdlib, not in the reference tree: tx_is_multicast
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "index_core.hpp"  // cidr_ok

#if defined(__HIPCC__)
#define NEB_RT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NEB_RT_HD inline
#endif

namespace neb {

// An address as two numbers: hi = bytes 0..7, lo = bytes 8..15, big-endian, so that a prefix is a
// mask of leading bits. A v4 address is its 32 bits at the top of hi. The family is kept beside it.
struct TxAddr {
    uint64_t hi, lo;
};
NEB_RT_HD bool tx_addr_eq(const TxAddr& a, const TxAddr& b) { return ((a.hi ^ b.hi) | (a.lo ^ b.lo)) == 0; }
NEB_RT_HD TxAddr tx_prefix_mask(uint32_t bits) {  // bits <= 128
    TxAddr m;
    m.hi = bits == 0 ? 0 : bits >= 64 ? ~0ull : ~0ull << (64 - bits);
    m.lo = bits <= 64 ? 0 : bits >= 128 ? ~0ull : ~0ull << (128 - bits);
    return m;
}
inline TxAddr tx_addr_from_bytes(const uint8_t* b, uint32_t family) {
    TxAddr a{0, 0};
    for (uint32_t i = 0; i < (family == 4 ? 4u : 16u); i++) {
        if (i < 8) a.hi |= (uint64_t)b[i] << (56 - 8 * i);
        else a.lo |= (uint64_t)b[i] << (120 - 8 * i);
    }
    return a;
}

// One slot of the open-addressing table (linear probing over a power-of-two number of slots, at
// least 4 x the capacity), the index table's scheme (index_core.hpp, IdxSlot) with a wider key: the
// tag carries kind, family, prefix length and 48 bits of the key's hash, the address words the
// key itself. Within one image a slot only moves EMPTY -> LIVE -> TOMBSTONE, or EMPTY -> TOMBSTONE;
// addr_lo, addr_hi and value are written once, before the tag says LIVE, and never again. A search
// compares the tag and then the address words. A replace puts the new record into the next EMPTY
// slot of the chain (always behind the old one) and then tombstones the old one.
struct TxSlot {
    uint64_t tag;  // kTxEmpty, kTxTomb or tx_tag(...)
    uint64_t addr_lo, addr_hi;
    uint64_t value;  // HOST: the tunnel; ROUTE: first gateway | gateway count << 32
};
static_assert(sizeof(TxSlot) == 32, "a slot never straddles a 64-byte line");
constexpr uint64_t kTxEmpty = 0, kTxTomb = 1;

// A gateway of a route: immutable per image.
struct TxGw {
    TxAddr addr;
    uint32_t family;
    uint32_t bound;  // bucketUpperBound
};
static_assert(sizeof(TxGw) == 24, "");

// The prefix lengths present among the routes: bit b of v4 (b <= 32); bit b & 63 of v6[b >> 6].
struct TxLens {
    uint64_t v4;
    uint64_t v6[3];
};

// The own networks as the gates and the lookup scan them.
struct TxOwn {
    uint32_t n, flags;
    uint32_t family[NEB_INDEX_MAX_NETWORKS];
    TxAddr addr[NEB_INDEX_MAX_NETWORKS];   // the own address (myVpnAddrsTable)
    TxAddr mask[NEB_INDEX_MAX_NETWORKS];   // the network's leading bits (myVpnNetworksTable)
    uint64_t bcast[NEB_INDEX_MAX_NETWORKS];  // family 4: network | ~mask, as TxAddr.hi
};

inline void tx_own_set(TxOwn* o, const neb_cidr* nets, uint32_t n, uint32_t flags) {
    *o = TxOwn{};
    o->n = n;
    o->flags = flags;
    for (uint32_t k = 0; k < n; k++) {
        o->family[k] = nets[k].family;
        o->addr[k] = tx_addr_from_bytes(nets[k].addr, nets[k].family);
        o->mask[k] = tx_prefix_mask(nets[k].bits);
        if (nets[k].family == 4) o->bcast[k] = (o->addr[k].hi | ~o->mask[k].hi) & 0xFFFFFFFF00000000ull;
    }
}

// The hash of an address and 64 bits of whatever else the key holds (also peer_core.hpp).
NEB_RT_HD uint64_t tx_mix(const TxAddr& a, uint64_t rest) {
    uint64_t x = a.hi ^ (a.lo * 0x9E3779B97F4A7C15ull) ^ (rest * 0xD6E8FEB86659FD93ull);
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ull;
    return x ^ (x >> 32);
}
NEB_RT_HD uint64_t tx_hash(uint32_t kind, uint32_t family, uint32_t bits, const TxAddr& a) {
    return tx_mix(a, (kind << 16) | (family << 8) | bits);
}
NEB_RT_HD uint64_t tx_tag(uint32_t kind, uint32_t family, uint32_t bits, uint64_t hash) {
    return (1ull << 63) | ((uint64_t)kind << 62) | ((uint64_t)(family == 6) << 61) | ((uint64_t)bits << 48) | (hash >> 16);
}
NEB_RT_HD uint32_t tx_slots_for(uint32_t entries) {  // entries <= 2^28
    uint32_t s = 16;
    while (s < 4u * entries) s <<= 1;
    return s;
}

// The search for the record with tag `want` and address a whose hash is h: walks the chain from the
// key's home slot to the key or to the first EMPTY slot. ld(p) reads one 64-bit word of the image.
// Reads a slot's words in program order: tag, then the address words. *slot: where it ended;
// *probes: slots examined.
template <class Load>
NEB_RT_HD bool tx_find_tag(const TxSlot* slots, uint32_t mask, uint64_t h, uint64_t want, const TxAddr& a, Load ld,
                           uint32_t* slot, uint32_t* probes) {
    uint32_t s = (uint32_t)h & mask;
    for (uint32_t k = 1; k <= mask + 1u; k++, s = (s + 1u) & mask) {
        const uint64_t t = ld(&slots[s].tag);
        bool hit = t == want;
        if (hit) {
            const uint64_t lo = ld(&slots[s].addr_lo), hi = ld(&slots[s].addr_hi);
            hit = lo == a.lo && hi == a.hi;
        }
        if (hit || t == kTxEmpty) {
            *slot = s;
            *probes = k;
            return hit;
        }
    }
    *slot = s;
    *probes = mask + 1u;
    return false;
}
// The search for (kind, family, bits, a).
template <class Load>
NEB_RT_HD bool tx_find(const TxSlot* slots, uint32_t mask, uint32_t kind, uint32_t family, uint32_t bits,
                       const TxAddr& a, Load ld, uint32_t* slot, uint32_t* probes) {
    const uint64_t h = tx_hash(kind, family, bits, a);
    return tx_find_tag(slots, mask, h, tx_tag(kind, family, bits, h), a, ld, slot, probes);
}
template <class Load>
NEB_RT_HD bool tx_lookup(const TxSlot* slots, uint32_t mask, uint32_t kind, uint32_t family, uint32_t bits,
                         const TxAddr& a, Load ld, uint64_t* value) {
    uint32_t s, probes;
    if (!tx_find(slots, mask, kind, family, bits, a, ld, &s, &probes)) return false;
    *value = ld(&slots[s].value);
    return true;
}

// ---- newPacket(data, incoming, fp) ----------------------------------------------------------------

struct TxParsed {
    TxAddr local, remote;
    uint32_t family;  // 4 | 6
    uint32_t local_port, remote_port, protocol;
    uint32_t flags;       // NEB_FW_FRAGMENT | NEB_FW_FRAG_ANY
    uint32_t ip_hdr_len;  // IPHdrLen
};

// byte(i): byte i of the packet, called for i < len only. false: newPacket's error; ip_hdr_len and
// NEB_FW_FRAG_ANY are then as newPacket had left them and every other field is zero. kIncoming: the
// record is locally oriented, so the source is the remote side, for addresses and ports; the ICMP /
// ICMPv6-echo identifier is remote_port either way (outside.go:345-351, 378-399, 449-469).
template <bool kIncoming = false, class Byte>
NEB_RT_HD bool tx_new_packet(uint32_t len, Byte byte, TxParsed* p) {
    auto be16 = [&](uint32_t i) { return (byte(i) << 8) | byte(i + 1u); };
    auto be32 = [&](uint32_t i) { return ((uint64_t)be16(i) << 16) | be16(i + 2u); };
    auto be64 = [&](uint32_t i) { return (be32(i) << 32) | be32(i + 4u); };
    *p = TxParsed{};
    if (len < 1u) return false;  // ErrPacketTooShort
    const uint32_t b0 = byte(0u);
    if ((b0 >> 4) == 4u) {  // parseV4
        if (len < 20u) return false;
        const uint32_t ihl = (b0 & 15u) << 2;
        if (ihl < 20u) return false;
        const uint32_t ff = be16(6u);
        const bool fragment = (ff & 0x1FFFu) != 0u;
        if (ff & 0x3FFFu) p->flags = NEB_FW_FRAG_ANY;
        p->ip_hdr_len = ihl;
        const uint32_t proto = byte(9u);
        // minFwPacketLen = 4: the ports; ICMP reads the identifier at +4..+6
        if (len < ihl + (fragment ? 0u : proto == 1u ? 6u : 4u)) return false;
        p->protocol = proto;
        p->family = 4u;
        p->local = TxAddr{be32(kIncoming ? 16u : 12u) << 32, 0};
        p->remote = TxAddr{be32(kIncoming ? 12u : 16u) << 32, 0};
        if (fragment) {
            p->flags |= NEB_FW_FRAGMENT;
        } else if (proto == 1u) {
            p->remote_port = be16(ihl + 4u);
        } else {
            p->local_port = be16(ihl + (kIncoming ? 2u : 0u));
            p->remote_port = be16(ihl + (kIncoming ? 0u : 2u));
        }
        return true;
    }
    if ((b0 >> 4) != 6u) return false;  // ErrUnknownIPVersion
    if (len < 40u) return false;        // parseV6
    // IPv6FindUpperProtocol: at most 8 extension headers; the protocol after them is reported as is
    uint32_t nh = byte(6u), off = 40u;
    bool is_frag = false, any_frag = false;
    for (int k = 0; k < 8; k++) {
        if (nh == 0u || nh == 43u || nh == 60u) {  // hop-by-hop, routing, destination options
            if (len < off + 2u) return false;
            nh = byte(off);
            off += (byte(off + 1u) + 1u) << 3;
        } else if (nh == 44u) {  // fragment
            if (len < off + 8u) return false;
            any_frag = true;
            if (byte(off + 2u) != 0u || (byte(off + 3u) & 0xF8u) != 0u) {  // a non-first fragment ends the walk
                nh = byte(off);
                is_frag = true;
                break;
            }
            nh = byte(off);
            off += 8u;
        } else if (nh == 51u) {  // AH
            if (len < off + 2u) return false;
            nh = byte(off);
            off += (byte(off + 1u) + 2u) << 2;
        } else {
            if (off > len) return false;
            break;
        }
    }
    p->ip_hdr_len = off;
    p->flags = any_frag ? NEB_FW_FRAG_ANY : 0u;
    if (!is_frag) {
        if (nh == 58u) {  // ICMPv6: type, code, checksum; echo request / reply carry the identifier
            if (len < off + 4u) return false;
            const uint32_t type = byte(off);
            if (type == 128u || type == 129u) {
                if (len < off + 6u) return false;
                p->remote_port = be16(off + 4u);
            }
        } else if (nh == 6u || nh == 17u) {
            if (len < off + 4u) return false;
            p->local_port = be16(off + (kIncoming ? 2u : 0u));
            p->remote_port = be16(off + (kIncoming ? 0u : 2u));
        }
    } else {
        p->flags |= NEB_FW_FRAGMENT;
    }
    p->protocol = nh;
    p->family = 6u;
    p->local = TxAddr{be64(kIncoming ? 24u : 8u), be64(kIncoming ? 32u : 16u)};
    p->remote = TxAddr{be64(kIncoming ? 8u : 24u), be64(kIncoming ? 16u : 32u)};
    return true;
}

// ---- the gates ------------------------------------------------------------------------------------

// [ext] netip.Addr.IsMulticast: 224.0.0.0/4, ff00::/8, a 4-in-6 address unmapped first.
NEB_RT_HD bool tx_is_multicast(uint32_t family, const TxAddr& a) {
    if (family == 4u) return (a.hi >> 60) == 0xEu;
    if (a.hi == 0u && (a.lo >> 32) == 0xFFFFu) return ((a.lo >> 28) & 0xFu) == 0xEu;
    return (a.hi >> 56) == 0xFFu;
}

// 0, or the NEB_FW_GATE_* flag of the first gate that drops the packet (inside.go:43-76).
NEB_RT_HD uint32_t tx_gates(const TxOwn& own, uint32_t family, const TxAddr& remote, bool* in_network) {
    bool bcast = false, self = false, inside = false;
    for (uint32_t k = 0; k < own.n; k++) {
        const bool fam = own.family[k] == family;
        bcast |= fam && family == 4u && remote.hi == own.bcast[k];
        self |= fam && tx_addr_eq(remote, own.addr[k]);
        inside |= fam && (((remote.hi ^ own.addr[k].hi) & own.mask[k].hi) | ((remote.lo ^ own.addr[k].lo) & own.mask[k].lo)) == 0u;
    }
    *in_network = inside;
    if ((own.flags & NEB_TX_DROP_LOCAL_BROADCAST) && bcast) return NEB_FW_GATE_BROADCAST;
    if (self) return NEB_FW_GATE_SELF;
    if ((own.flags & NEB_TX_DROP_MULTICAST) && tx_is_multicast(family, remote)) return NEB_FW_GATE_MULTICAST;
    return 0u;
}

// ---- ECMP -----------------------------------------------------------------------------------------

NEB_RT_HD uint32_t tx_hash_packet(uint32_t local_port, uint32_t remote_port) {  // hashPacket
    uint32_t x = (local_port << 16) | remote_port;
    x ^= x >> 16;
    x *= 0x21F0AAADu;
    x ^= x >> 15;
    x *= 0xD35A2D97u;
    x ^= x >> 15;
    return x & 0x7FFFFFFFu;
}
// CalculateBucketsForGateways: the upper bound of the bucket that ends at cumulative weight `upto`.
inline uint32_t tx_bucket_bound(uint64_t upto, uint64_t total) {  // total > 0, upto <= total < 2^32
    return (uint32_t)(((upto << 31) + total / 2) / total) - 1u;
}

// ---- longest prefix -------------------------------------------------------------------------------

// RoutesFor's method (also peer_core.hpp): one probe per prefix length present, the longest first.
// probe(bits, masked address) -> found.
template <class Probe>
NEB_RT_HD bool tx_longest_prefix(const TxLens& lens, uint32_t family, const TxAddr& a, Probe probe) {
    bool found = false;
    auto scan = [&](uint64_t m, uint32_t base) {  // the lengths base + 63 .. base that are present
        while (m && !found) {
            const uint32_t b = 63u - (uint32_t)__builtin_clzll(m);
            m &= ~(1ull << b);
            const TxAddr pm = tx_prefix_mask(base + b);
            found = probe(base + b, TxAddr{a.hi & pm.hi, a.lo & pm.lo});
        }
    };
    if (family == 4u) {
        scan(lens.v4, 0u);
    } else {
        scan(lens.v6[2], 128u);
        scan(lens.v6[1], 64u);
        scan(lens.v6[0], 0u);
    }
    return found;
}
inline void tx_lens_add(TxLens* l, uint32_t family, uint32_t bits) {
    if (family == 4) l->v4 |= 1ull << bits;
    else l->v6[bits >> 6] |= 1ull << (bits & 63u);
}

// ---- the resolve of one TUN read ------------------------------------------------------------------

struct TxResult {
    uint32_t tunnel;
    int32_t status;
    uint32_t fw[12];  // neb_fw_packet as little-endian dwords
};
NEB_RT_HD uint32_t tx_bswap(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
NEB_RT_HD void tx_addr_words(const TxAddr& a, uint32_t* w) {  // the 16 address bytes
    w[0] = tx_bswap((uint32_t)(a.hi >> 32));
    w[1] = tx_bswap((uint32_t)a.hi);
    w[2] = tx_bswap((uint32_t)(a.lo >> 32));
    w[3] = tx_bswap((uint32_t)a.lo);
}

// byte(i): the packet. look(kind, family, bits, addr, &value): the table. gw(i): gateway i.
template <class Byte, class Look, class Gw>
NEB_RT_HD void tx_resolve_one(uint32_t len, Byte byte, const TxOwn& own, const TxLens& lens, Look look, Gw gw,
                              TxResult* out) {
    // a failed parse leaves p zero but for ip_hdr_len and NEB_FW_FRAG_ANY: the record is built below
    TxParsed p;
    const bool parsed = tx_new_packet(len, byte, &p);
    out->tunnel = NEB_TX_NO_TUNNEL;
    uint32_t flags = p.flags, gateway = parsed ? NEB_GATEWAY_NONE : 0u;
    int32_t status = parsed ? NEB_STATUS_OK : NEB_STATUS_INVALID;
    uint64_t v = 0;
    bool in_network = false;
    const uint32_t gate = parsed ? tx_gates(own, p.family, p.remote, &in_network) : 0u;
    if (!parsed) {
        // a silent drop
    } else if (gate) {
        flags |= gate;
        status = NEB_STATUS_TX_DROPPED;
    } else if (in_network) {  // getOrHandshakeNoRouting: the pending hostinfo is not nil, no routing
        if (look((uint32_t)NEB_TX_KIND_HOST, p.family, 0u, p.remote, &v)) out->tunnel = (uint32_t)v;
        else status = NEB_STATUS_NO_TUNNEL;
    } else {
        const bool found = tx_longest_prefix(lens, p.family, p.remote, [&](uint32_t bits, const TxAddr& masked) {
            return look((uint32_t)NEB_TX_KIND_ROUTE, p.family, bits, masked, &v);
        });
        if (!found) {
            status = NEB_STATUS_NO_ROUTE;
        } else {
            flags |= NEB_FW_ROUTED;
            const uint32_t first = (uint32_t)v, count = (uint32_t)(v >> 32);
            uint32_t pick = 0;
            if (count > 1u) {  // BalancePacket: the last bound is 2^31 - 1, so one always matches
                const uint32_t h = tx_hash_packet(p.local_port, p.remote_port);
                while (pick + 1u < count && h > gw(first + pick).bound) pick++;
            }
            gateway = first + pick;
            const TxGw g = gw(gateway);
            if (look((uint32_t)NEB_TX_KIND_HOST, g.family, 0u, g.addr, &v)) {
                out->tunnel = (uint32_t)v;
            } else {
                status = NEB_STATUS_NO_TUNNEL;
                for (uint32_t k = 0; k < count && count > 1u; k++) {  // inside.go:355-365
                    const TxGw o = gw(first + k);
                    if (o.family == g.family && tx_addr_eq(o.addr, g.addr)) continue;
                    if (look((uint32_t)NEB_TX_KIND_HOST, o.family, 0u, o.addr, &v)) {
                        out->tunnel = (uint32_t)v;
                        flags |= NEB_FW_ECMP_FALLBACK;
                        status = NEB_STATUS_OK;
                        break;
                    }
                }
            }
        }
    }
    out->status = status;
    tx_addr_words(p.local, out->fw);
    tx_addr_words(p.remote, out->fw + 4);
    out->fw[8] = p.local_port | (p.remote_port << 16);
    out->fw[9] = p.protocol | (p.family << 8) | (flags << 16);
    out->fw[10] = p.ip_hdr_len;
    out->fw[11] = gateway;
}

}  // namespace neb
