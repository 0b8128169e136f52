// index_core.hpp — the rules of the receive resolve (neb_index_table_*, neb_rx_resolve_batch),
// shared by the host table and host form (index.cpp), the device form (resolve.hip) and the
// sanitizer program (tests/sanitize_index). Plain C++17; compiles with g++ alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   the double-encryption check            outside.go:66-74  (myVpnNetworksTable.Contains)
//   the tunnel of a header's remote index  outside.go:93-106, hostmap.go:546-577
//   the relay's type and target            outside.go:201-240
//   netip.Prefix.Contains                  a v4 address only in v4 prefixes, 4-in-6 only in v6 ones
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"

#if defined(__HIPCC__)
#define NEB_IDX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NEB_IDX_HD inline
#endif

namespace neb {

// One slot of the open-addressing table (linear probing over a power-of-two number of slots, at
// least 4 x capacity). Within one image a slot only moves EMPTY -> LIVE -> TOMBSTONE, or EMPTY ->
// TOMBSTONE; a, b are written once, before the tag says LIVE, and never again. A replace puts the
// new record into the next EMPTY slot of the chain (always behind the old one) and then tombstones
// the old one, so a search that walks the chain while that happens meets one of the two. Tombstones
// are not reused; a rebuild into the other image drops them.
struct IdxSlot {
    uint64_t tag;  // kIdxEmpty, kIdxTomb or idx_tag(space, index)
    uint64_t a;    // key_id | flags << 32
    uint64_t b;    // route.tunnel | route.remote_index << 32
    uint64_t pad;
};
static_assert(sizeof(IdxSlot) == 32, "a slot never straddles a 64-byte line");
constexpr uint64_t kIdxEmpty = 0, kIdxTomb = 1;

struct IdxRec {
    uint32_t key_id, flags;
    neb_relay_route route;
};

NEB_IDX_HD uint64_t idx_tag(uint32_t space, uint32_t index) {
    return (1ull << 63) | ((uint64_t)space << 32) | index;
}
NEB_IDX_HD uint32_t idx_hash(uint32_t space, uint32_t index) {
    uint32_t h = (index ^ (space * 0x85EBCA6Bu)) * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    return h ^ (h >> 13);
}
NEB_IDX_HD uint64_t idx_pack_a(const neb_index_entry& e) { return e.key_id | ((uint64_t)e.flags << 32); }
NEB_IDX_HD uint64_t idx_pack_b(const neb_index_entry& e) {
    return e.route.tunnel | ((uint64_t)e.route.remote_index << 32);
}
NEB_IDX_HD uint32_t idx_slots_for(uint32_t capacity) {  // capacity <= 2^28
    uint32_t s = 16;
    while (s < 4u * capacity) s <<= 1;
    return s;
}

// The search for (space, index): walks the chain from the key's home slot to the key or to the
// first EMPTY slot. ld(p) reads one 64-bit word of the image. *slot: where it ended; *probes: slots
// examined. The table always keeps EMPTY slots; the bound only guards a damaged image.
template <class Load>
NEB_IDX_HD bool idx_find(const IdxSlot* slots, uint32_t mask, uint32_t space, uint32_t index, Load ld,
                                uint32_t* slot, uint32_t* probes) {
    const uint64_t want = idx_tag(space, index);
    uint32_t s = idx_hash(space, index) & mask;
    for (uint32_t k = 1; k <= mask + 1u; k++, s = (s + 1u) & mask) {
        const uint64_t t = ld(&slots[s].tag);
        if (t == want || t == kIdxEmpty) {
            *slot = s;
            *probes = k;
            return t == want;
        }
    }
    *slot = s;
    *probes = mask + 1u;
    return false;
}

template <class Load>
NEB_IDX_HD bool idx_lookup(const IdxSlot* slots, uint32_t mask, uint32_t space, uint32_t index, Load ld,
                                  bool want_route, IdxRec* r) {
    uint32_t s, probes;
    if (!idx_find(slots, mask, space, index, ld, &s, &probes)) return false;
    const uint64_t a = ld(&slots[s].a);
    r->key_id = (uint32_t)a;
    r->flags = (uint32_t)(a >> 32);
    r->route = neb_relay_route{NEB_RELAY_NONE, 0};
    if (want_route) {
        const uint64_t b = ld(&slots[s].b);
        r->route = neb_relay_route{(uint32_t)b, (uint32_t)(b >> 32)};
    }
    return true;
}

// ---- own networks ----------------------------------------------------------------------------

// The prefixes as the resolve scans them: per prefix the address and the mask of its leading bits,
// as the four little-endian dwords of their 16 bytes (a v4 prefix uses the first only).
struct IdxNets {
    uint32_t n;
    uint32_t family[NEB_INDEX_MAX_NETWORKS];
    uint32_t addr[NEB_INDEX_MAX_NETWORKS][4];
    uint32_t mask[NEB_INDEX_MAX_NETWORKS][4];
};

// A prefix the tables take (both; route_core.hpp): a family, and no more bits than it has.
inline bool cidr_ok(const neb_cidr& c) {
    return (c.family == 4 && c.bits <= 32) || (c.family == 6 && c.bits <= 128);
}
inline void idx_nets_set(IdxNets* out, const neb_cidr* nets, uint32_t n) {
    *out = IdxNets{};
    out->n = n;
    for (uint32_t k = 0; k < n; k++) {
        out->family[k] = nets[k].family;
        for (uint32_t b = 0; b < 16; b++) {
            const int keep = (int)nets[k].bits - 8 * (int)b;
            const uint32_t m = keep >= 8 ? 0xFFu : keep <= 0 ? 0u : (0xFF00u >> keep) & 0xFFu;
            out->mask[k][b >> 2] |= m << (8 * (b & 3));
            out->addr[k][b >> 2] |= (nets[k].addr[b] & m) << (8 * (b & 3));
        }
    }
}
// netip.Prefix.Contains over the set; a: the address bytes as little-endian dwords.
NEB_IDX_HD bool idx_own_source(const IdxNets& nets, uint32_t family, const uint32_t a[4]) {
    bool hit = false;
    for (uint32_t k = 0; k < nets.n; k++) {
        uint32_t d = (a[0] & nets.mask[k][0]) ^ nets.addr[k][0];
        if (family == 6)
            d |= ((a[1] & nets.mask[k][1]) ^ nets.addr[k][1]) | ((a[2] & nets.mask[k][2]) ^ nets.addr[k][2]) |
                 ((a[3] & nets.mask[k][3]) ^ nets.addr[k][3]);
        hit |= nets.family[k] == family && d == 0;
    }
    return hit;
}

// ---- the resolve of one packet ----------------------------------------------------------------

NEB_IDX_HD uint32_t idx_rx_len(const neb_rx_packet& p) { return p.len & ~NEB_RX_OWN_SOURCE; }
NEB_IDX_HD uint32_t idx_bswap(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
// The two fields of a header the lookups need, from its bytes 0:4 and 4:8 as little-endian dwords:
// Message (type 1, any version) with subtype MessageRelay, and the remote index.
NEB_IDX_HD void idx_header(uint32_t w0, uint32_t w1, bool* relay, uint32_t* index) {
    *relay = (w0 & 15u) == 1u && ((w0 >> 8) & 255u) == 1u;
    *index = idx_bswap(w1);
}

// hdr(at, &w0, &w1): bytes 0:8 of the header at off + at (at = 0 or 16; called only where the
// packet holds those 16 bytes). look(space, index, want_route, &rec): the table.
template <class Hdr, class Look>
NEB_IDX_HD void idx_resolve_one(uint32_t len, Hdr hdr, Look look, uint32_t* key, neb_relay_route* route,
                                neb_rx_via* via) {
    uint32_t k = NEB_KEYS_MIXED, inner = NEB_KEYS_MIXED, flags = 0;
    neb_relay_route rt{NEB_RELAY_NONE, 0};
    if (len >= 16u) {
        uint32_t w0, w1, index;
        bool relay;
        hdr(0u, &w0, &w1);
        idx_header(w0, w1, &relay, &index);
        IdxRec r;
        if (look(relay ? (uint32_t)NEB_INDEX_RELAY : (uint32_t)NEB_INDEX_TUNNEL, index, relay, &r)) {
            k = r.key_id;
            if (relay && r.route.tunnel != NEB_RELAY_NONE) rt = r.route;
            if (relay && (r.flags & NEB_VIA_TERMINAL)) {
                flags = NEB_VIA_TERMINAL;
                if (len >= 48u) {
                    hdr(16u, &w0, &w1);
                    idx_header(w0, w1, &relay, &index);
                    IdxRec in;
                    if (look(relay ? (uint32_t)NEB_INDEX_RELAY : (uint32_t)NEB_INDEX_TUNNEL, index, false, &in))
                        inner = in.key_id;
                }
            }
        }
    }
    *key = k;
    *route = rt;
    *via = neb_rx_via{inner, flags};
}

}  // namespace neb
