// peer_core.hpp — the rules of the RX inner resolve (neb_peer_table_*, neb_rx_inner_batch), shared by
// the host table and host form (peer.cpp), the device form (peer.hip) and the sanitizer program
// (tests/sanitize_peer). Plain C++17; compiles with g++ alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   handleOutsideMessagePacket             outside.go:474-494
//   newPacket(data, true, fp)              outside.go:320-472 (route_core.hpp, tx_new_packet<true>)
//   firewall.Drop, the two address checks  firewall.go:425-457
//   HostInfo.buildNetworks                 hostmap.go:837-857 (the caller's, nebula_amd/hostmap.py)
//   routableNetworks                       firewall.go:154-165
//   netip.Prefix.Contains                  a v4 address only in v4 prefixes, 4-in-6 only in v6 ones
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "route_core.hpp"  // TxAddr, TxSlot, TxLens, tx_mix, tx_find_tag, tx_longest_prefix, tx_new_packet

namespace neb {

// The table's slots are the TX table's (TxSlot: tag, address words, value; the same life cycle, the
// same scatter). The tag carries family, prefix length, 16 bits of the key's hash and the tunnel
// itself, so a tag that matches has compared the tunnel; the address words are the masked prefix;
// the value is the NEB_NET_* type.
NEB_RT_HD uint64_t peer_hash(uint32_t tunnel, uint32_t family, uint32_t bits, const TxAddr& a) {
    return tx_mix(a, ((uint64_t)tunnel << 16) | (family << 8) | bits);
}
NEB_RT_HD uint64_t peer_tag(uint32_t tunnel, uint32_t family, uint32_t bits, uint64_t hash) {
    return (1ull << 63) | ((uint64_t)(family == 6) << 61) | ((uint64_t)bits << 48) | ((hash >> 48) << 32) | tunnel;
}
template <class Load>
NEB_RT_HD bool peer_find(const TxSlot* slots, uint32_t mask, uint32_t tunnel, uint32_t family, uint32_t bits,
                         const TxAddr& a, Load ld, uint32_t* slot, uint32_t* probes) {
    const uint64_t h = peer_hash(tunnel, family, bits, a);
    return tx_find_tag(slots, mask, h, peer_tag(tunnel, family, bits, h), a, ld, slot, probes);
}

// The routable set as the local check scans it: the masked network and the mask of its leading bits.
struct PeerRoutable {
    uint32_t n;
    uint32_t family[NEB_RX_MAX_ROUTABLE];
    TxAddr addr[NEB_RX_MAX_ROUTABLE];
    TxAddr mask[NEB_RX_MAX_ROUTABLE];
};
static_assert(sizeof(PeerRoutable) <= 2048, "travels in the kernel arguments, which end at 4 KiB");

inline void peer_routable_set(PeerRoutable* o, const neb_cidr* nets, uint32_t n) {
    *o = PeerRoutable{};
    o->n = n;
    for (uint32_t k = 0; k < n; k++) {
        const TxAddr a = tx_addr_from_bytes(nets[k].addr, nets[k].family), m = tx_prefix_mask(nets[k].bits);
        o->family[k] = nets[k].family;
        o->mask[k] = m;
        o->addr[k] = TxAddr{a.hi & m.hi, a.lo & m.lo};
    }
}
NEB_RT_HD bool peer_routable_contains(const PeerRoutable& r, uint32_t family, const TxAddr& a) {
    bool hit = false;
    for (uint32_t k = 0; k < r.n; k++)
        hit |= r.family[k] == family && (((a.hi & r.mask[k].hi) ^ r.addr[k].hi) | ((a.lo & r.mask[k].lo) ^ r.addr[k].lo)) == 0u;
    return hit;
}

// ---- one opened packet --------------------------------------------------------------------------

struct PeerResult {
    int32_t status;
    uint32_t plain[8];  // neb_plain_packet as little-endian dwords
    uint32_t fw[12];    // neb_fw_packet
};

// len: pk.len without NEB_RX_OWN_SOURCE. hdr(i): byte i of the 16-byte header, called only when
// len >= 32; body(i): byte i of the len - 32 plaintext bytes at off + 16; epoch(key_id): called
// for key_id < nepoch; look(family, bits, masked address, &type): the tunnel key_id's entry.
template <class Hdr, class Body, class Epoch, class Look>
NEB_RT_HD void peer_inner_one(uint64_t off, uint32_t len, uint32_t key_id, int32_t open_status, uint32_t nepoch,
                              Hdr hdr, Body body, Epoch epoch, const TxLens& lens, const PeerRoutable& routable,
                              Look look, PeerResult* out) {
    for (int k = 0; k < 8; k++) out->plain[k] = 0;
    for (int k = 0; k < 12; k++) out->fw[k] = 0;
    out->plain[7] = (uint32_t)NEB_PLAIN_SKIP << 24;
    out->status = NEB_STATUS_NOT_MESSAGE;
    // neb_rx_plain_from_wire's rule: header type Message, subtype None (outside.go:145-149)
    if (open_status != NEB_STATUS_OK || len < 32u || key_id >= nepoch) return;
    if ((hdr(0u) & 15u) != 1u || hdr(1u) != 0u) return;

    TxParsed p;
    const uint32_t plen = len - 32u;
    const bool parsed = tx_new_packet<true>(plen, body, &p);
    int32_t status = NEB_STATUS_INVALID;
    if (parsed) {
        uint64_t type = 0;
        const bool found = tx_longest_prefix(lens, p.family, p.remote, [&](uint32_t bits, const TxAddr& masked) {
            return look(p.family, bits, masked, &type);
        });
        if (!found) status = NEB_STATUS_RX_BAD_REMOTE;
        else if (type == NEB_NET_VPN_PEER) status = NEB_STATUS_RX_PEER_REJECTED;
        else if (!peer_routable_contains(routable, p.family, p.local)) status = NEB_STATUS_RX_BAD_LOCAL;
        else status = NEB_STATUS_OK;
    }
    out->status = status;
    tx_addr_words(p.local, out->fw);
    tx_addr_words(p.remote, out->fw + 4);
    out->fw[8] = p.local_port | (p.remote_port << 16);
    out->fw[9] = p.protocol | (p.family << 8) | (p.flags << 16);
    out->fw[10] = p.ip_hdr_len;
    out->fw[11] = parsed ? NEB_GATEWAY_NONE : 0u;
    if (status != NEB_STATUS_OK) return;

    const uint64_t at = off + 16u, ep = epoch(key_id);
    auto be32 = [&](uint32_t i) { return (hdr(i) << 24) | (hdr(i + 1u) << 16) | (hdr(i + 2u) << 8) | hdr(i + 3u); };
    out->plain[0] = (uint32_t)at;
    out->plain[1] = (uint32_t)(at >> 32);
    out->plain[2] = (uint32_t)ep;
    out->plain[3] = (uint32_t)(ep >> 32);
    out->plain[4] = be32(12u);  // counter = header bytes 8:16, big-endian
    out->plain[5] = be32(8u);
    out->plain[6] = plen;
    const uint32_t flags = NEB_PLAIN_PARSED | ((p.flags & NEB_FW_FRAG_ANY) ? NEB_PLAIN_FRAG_ANY : 0u);
    out->plain[7] = (p.ip_hdr_len & 0xFFFFu) | (p.protocol << 16) | (flags << 24);
}

}  // namespace neb
