// recv_core.hpp — the rules of the RX receive plan, shared by the host form (recv.cpp), the device
// form (recv.hip) and the sanitizer program (tests/sanitize_recv). Plain C++17; compiles with g++
// alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   getFrom            udp/udp_linux.go:237-246
//   deliverSegments    udp/udp_linux.go:291-303
//   parseRecvCmsg      udp/udp_linux.go:307-331
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nebula_aead.h"

#if defined(__HIPCC__)
#define NEB_RECV_HD __host__ __device__
#else
#define NEB_RECV_HD
#endif

namespace neb {

constexpr uint32_t kRecvMaxCtrlStride = 1024;  // the largest ctrl_stride accepted
constexpr uint32_t kRecvCmsgHdr = 16;          // SizeofCmsghdr = CmsgLen(0), Linux LP64
constexpr int32_t kRecvSolUdp = 17, kRecvUdpGro = 104;
constexpr uint32_t kRecvGroPayload = 4;  // udpGROCmsgPayload

static_assert(sizeof(neb_recv_entry) == 48 && offsetof(neb_recv_entry, name) == 16 &&
                  offsetof(neb_recv_entry, ctrl_len) == 44,
              "");
static_assert(sizeof(neb_rx_packet) == 16 && sizeof(neb_rx_source) == 20 && sizeof(neb_udp_addr) == 20, "");

// Loads from the control slot. The slot and every offset of the walk are multiples of 8 (the ABI's
// alignment, align8 steps), which the device form's loads rely on.
template <typename T>
NEB_RECV_HD inline T recv_load(const uint8_t* p) {
    T v;
    memcpy(&v, __builtin_assume_aligned(p, sizeof(T) < 8 ? 4 : 8), sizeof(T));
    return v;
}

// parseRecvCmsg over ctrl[0, L): the UDP_GRO size, or 0 when there is none. Reads no byte at or
// past L, whatever the lengths inside say.
NEB_RECV_HD inline int32_t recv_cmsg_walk(const uint8_t* ctrl, uint32_t L) {
    int32_t gso = 0;
    uint32_t off = 0;
    while (off + kRecvCmsgHdr <= L) {
        const int64_t clen = (int64_t)recv_load<uint64_t>(ctrl + off);  // the reference's int(ch.Len)
        // against the remaining bytes, not off + clen: that sum wraps for a length near the largest int
        if (clen < (int64_t)kRecvCmsgHdr || clen > (int64_t)(L - off)) return gso;
        if (recv_load<int32_t>(ctrl + off + 8) == kRecvSolUdp && recv_load<int32_t>(ctrl + off + 12) == kRecvUdpGro &&
            off + kRecvCmsgHdr + kRecvGroPayload <= L)
            gso = recv_load<int32_t>(ctrl + off + kRecvCmsgHdr);
        off += ((uint32_t)clen + 7u) & ~7u;  // CmsgSpace(clen - CmsgLen(0)); clen <= L - off <= 1024
    }
    return gso;
}

// The control slot of entry j clipped to the stride, then the walk.
NEB_RECV_HD inline int32_t recv_seg_size(const neb_recv_entry& en, const uint8_t* ctrl, uint32_t ctrl_stride, uint32_t j) {
    if (!ctrl) return en.seg_size;
    const uint32_t L = en.ctrl_len < ctrl_stride ? en.ctrl_len : ctrl_stride;
    return recv_cmsg_walk(ctrl + (size_t)j * ctrl_stride, L);
}

// deliverSegments: is the payload delivered whole?
NEB_RECV_HD inline bool recv_whole(uint32_t len, int32_t seg) { return seg <= 0 || (uint32_t)seg >= len; }

// The packets of an entry: at least one, at most 2^32 - 1.
NEB_RECV_HD inline uint64_t recv_count(uint32_t len, int32_t seg) {
    if (recv_whole(len, seg)) return 1u;
    return ((uint64_t)len + (uint32_t)seg - 1u) / (uint32_t)seg;
}

// Packet k < recv_count of an entry.
NEB_RECV_HD inline void recv_packet(uint64_t off, uint32_t len, int32_t seg, uint64_t k, uint64_t* p_off, uint32_t* p_len) {
    if (recv_whole(len, seg)) {
        *p_off = off;
        *p_len = len;
        return;
    }
    const uint64_t at = k * (uint32_t)seg, rest = len - at;
    *p_off = off + at;
    *p_len = rest < (uint32_t)seg ? (uint32_t)rest : (uint32_t)seg;
}

// getFrom. name: msg_name's 28 bytes as seven little-endian words (the entry is 8-byte aligned and
// name is at 16). a[0..4): the unmapped address, family 4 in a[0] with the rest zero.
struct RecvFrom {
    uint32_t a[4];
    uint32_t family;  // 4 | 6
    uint32_t port;
};
NEB_RECV_HD inline RecvFrom recv_from(const uint32_t name[7], uint32_t socket_v4) {
    RecvFrom f{};
    const uint32_t be = name[0] >> 16;  // name[2:4]
    f.port = ((be & 0xFFu) << 8) | (be >> 8);
    if (socket_v4) {
        f.a[0] = name[1];  // name[4:8]
        f.family = 4;
    } else if (name[2] == 0u && name[3] == 0u && name[4] == 0xFFFF0000u) {  // name[8:24] in ::ffff:0:0/96: Unmap
        f.a[0] = name[5];
        f.family = 4;
    } else {
        for (uint32_t k = 0; k < 4u; k++) f.a[k] = name[2u + k];
        f.family = 6;
    }
    return f;
}
// The last word of a neb_rx_source {family, reserved[3]} and of a neb_udp_addr {port, family, reserved}.
NEB_RECV_HD inline uint32_t recv_source_word(const RecvFrom& f) { return f.family; }
NEB_RECV_HD inline uint32_t recv_addr_word(const RecvFrom& f) { return f.port | (f.family << 16); }

// Is entry j emitted? first: the packets before it.
NEB_RECV_HD inline bool recv_emitted(uint64_t first, uint64_t count, uint32_t max_packets) {
    return first + count <= max_packets;  // first < 2^63, count < 2^32: no wrap
}

}  // namespace neb
