// send_core.hpp — the rules of the TX send plan, shared by the host form (send.cpp), the device form
// (send.hip) and the sanitizer program (tests/sanitize_send). Plain C++17; compiles with g++ alone
// (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   WriteBatch's packing loop, planRun     udp/udp_linux_writebatch.go:194-252, :312-346
//   writeSockaddr, Unmap on a v4 socket    udp/udp_linux.go:371-376
//   the destination of a wire              inside.go:178 (direct), :216 (relayHostInfo.GetRemote())
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nebula_aead.h"

#if defined(__HIPCC__)
#define NEB_SEND_HD __host__ __device__
#else
#define NEB_SEND_HD
#endif

namespace neb {

constexpr uint32_t kSendMaxSegments = 1024;  // the largest max_segments accepted
// The class of a wire in the plan.
enum : uint32_t {
    kSendAbsent = 0,      // NOT_SENT (or past *nwires): takes part in nothing, runs continue across it
    kSendRoutable = 1,    // one of WriteBatch's bufs that gets an iovec
    kSendUnroutable = 2,  // one of WriteBatch's bufs whose run is skipped: breaks runs, no iovec
    kSendBadKey = 3,      // a bad index: unroutable, with a destination no other wire has
};

// One wire as the plan sees it: its destination's 20 bytes as five words, its length, its
// destination tunnel and its class.
struct SendRec {
    uint32_t a[5];
    uint32_t len;
    uint32_t dst;
    uint32_t cls;
};
static_assert(sizeof(neb_udp_addr) == 20 && sizeof(SendRec) == 32, "");
static_assert(sizeof(neb_send_iov) == 16 && sizeof(neb_send_entry) == 16, "");

NEB_SEND_HD inline uint32_t send_family(const uint32_t a[5]) { return (a[4] >> 16) & 0xFFu; }

// Can the socket address it? Family 4 always; family 6 on a v6 socket, and on a v4 socket when it
// is ::ffff:0:0/96 (Unmap). Anything else, family 0 included, never.
NEB_SEND_HD inline bool send_routable(const uint32_t a[5], uint32_t socket_v4) {
    const uint32_t f = send_family(a);
    if (f == 4u) return true;
    if (f != 6u) return false;
    return !socket_v4 || (a[0] == 0u && a[1] == 0u && a[2] == 0xFFFF0000u);
}

// The wire -> destination step. `remote` is read once, as five words (its alignment is 2: memcpy).
NEB_SEND_HD inline void send_classify(const neb_tx_wire& w, int32_t wire_status, const neb_tx_packet* packets,
                                      uint32_t npackets, const neb_relay_route* via, const neb_udp_addr* remote,
                                      uint32_t ntunnels, uint32_t socket_v4, SendRec* r) {
    r->a[0] = r->a[1] = r->a[2] = r->a[3] = r->a[4] = 0;
    r->len = w.len;
    r->dst = NEB_SEND_NONE;
    r->cls = kSendAbsent;
    if (wire_status != NEB_STATUS_OK) return;
    r->cls = kSendBadKey;
    if (w.packet >= npackets) return;
    uint32_t t = packets[w.packet].tunnel;
    if (t >= ntunnels) return;
    if (w.reserved & NEB_TX_WIRE_VIA) {
        if (!via) return;
        t = via[t].tunnel;
        if (t >= ntunnels) return;
    }
    r->dst = t;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(&remote[t], 4));  // the ABI's rule
    for (uint32_t k = 0; k < 5u; k++) r->a[k] = p[k];
#else
    memcpy(r->a, &remote[t], sizeof(neb_udp_addr));
#endif
    r->cls = send_routable(r->a, socket_v4) ? kSendRoutable : kSendUnroutable;
}

NEB_SEND_HD inline int32_t send_status_of(uint32_t cls) {
    return cls == kSendRoutable     ? NEB_STATUS_OK
           : cls == kSendUnroutable ? NEB_STATUS_UNROUTABLE
           : cls == kSendBadKey     ? NEB_STATUS_BAD_KEY
                                    : NEB_STATUS_NOT_SENT;
}

NEB_SEND_HD inline bool send_same_dst(const SendRec& x, const SendRec& y) {
    return x.a[0] == y.a[0] && x.a[1] == y.a[1] && x.a[2] == y.a[2] && x.a[3] == y.a[3] && x.a[4] == y.a[4];
}

// max_segments <= 1: GSO is off, every packet is its own entry.
NEB_SEND_HD inline uint32_t send_max_segments(uint32_t max_segments) { return max_segments < 1u ? 1u : max_segments; }

// The most packets of length z one run of its plateau takes: planRun's two caps.
NEB_SEND_HD inline uint32_t send_run_cap(uint32_t z, uint32_t max_segments) {
    if (z == 0u || z > NEB_SEND_MAX_BYTES) return 1u;
    const uint32_t by_bytes = NEB_SEND_MAX_BYTES / z, ms = send_max_segments(max_segments);
    return by_bytes < ms ? by_bytes : ms;
}

// ---- the parallel form's two predicates (send.hip) ------------------------------------------------

// Does routable wire `cur` of rank `rank` start a hard segment? `prev` is the previous wire that is
// not absent (has_prev: there is one). A routable prev has rank - 1.
NEB_SEND_HD inline bool send_hard(bool has_prev, const SendRec& prev, const SendRec& cur, uint32_t rank,
                                  uint32_t chunk_packets) {
    if (!has_prev || prev.cls != kSendRoutable || !send_same_dst(prev, cur)) return true;
    if (cur.len == 0u || prev.len == 0u || prev.len > NEB_SEND_MAX_BYTES || cur.len > prev.len) return true;
    return chunk_packets != 0u && rank % chunk_packets == 0u;
}

// A plateau as a function {0,1} -> {0,1} in two bits (bit o = f(o)): o_j, "the run before took this
// plateau's first packet", to o_{j+1}. n, z: plateau j's packets and length; z_next: plateau j+1's.
constexpr uint32_t kSendFnIdentity = 2u, kSendFnZero = 0u;
NEB_SEND_HD inline uint32_t send_plateau_fn(uint32_t n, uint32_t z, uint32_t z_next, uint32_t max_segments) {
    const uint32_t ms = send_max_segments(max_segments), k = send_run_cap(z, max_segments);
    uint32_t f = 0;
    for (uint32_t o = 0; o < 2u; o++) {
        if (n <= o) continue;  // m == 0
        const uint32_t c = (n - o - 1u) % k + 1u;
        if (c < ms && (uint64_t)c * z + z_next <= NEB_SEND_MAX_BYTES) f |= 1u << o;
    }
    return f;
}
// x first, then y.
NEB_SEND_HD inline uint32_t send_fn_compose(uint32_t x, uint32_t y) {
    return ((y >> (x & 1u)) & 1u) | (((y >> ((x >> 1) & 1u)) & 1u) << 1);
}
// Does plateau position t start a run, given the plateau's o and cap k?
NEB_SEND_HD inline bool send_run_start(uint32_t t, uint32_t o, uint32_t k) { return t >= o && (t - o) % k == 0u; }

}  // namespace neb
