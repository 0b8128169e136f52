// relay.hpp — the forwarding half of a relay node's receive batch (relay.hip), shared with
// window.cpp: per-packet rules as one host/device inline, and the device workspace of the plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nebula_aead.h"
#include "layout.hpp"

namespace neb {

// Batches of at most this many packets are planned by one workgroup (relay_plan_small_kernel);
// larger ones by the grid-wide sort / scan-by-key form.
constexpr uint32_t kRelayPlanThreads = 1024, kRelayPlanItems = 8;
constexpr uint32_t kRelayPlanSmallMax = kRelayPlanThreads * kRelayPlanItems;

struct RelayWs {
    // per packet (arrival index)
    uint32_t* key;  // target tunnel of a packet that takes a counter, ntunnels for every other
    uint32_t* idx;
    // sorted by tunnel, arrival order kept (the grid-wide form)
    uint32_t* key_sorted;
    uint32_t* idx_sorted;
    uint32_t* rank;  // packets of the same tunnel earlier in the batch
    // forwarded packets, compacted: the AD-only seal's batch
    neb_desc* sub_desc;
    uint32_t* sub_map;  // arrival index
    int32_t* sub_status;
    uint32_t* nsub;
    uint32_t* tun_total;  // per tunnel: counters taken in this batch (the grid-wide form)
    void* cub_tmp;
    size_t cub_bytes;
};

inline size_t relay_align(size_t x) { return (x + 255) & ~(size_t)255; }

// Carve a RelayWs for n packets and ntun tunnels out of base (nullptr: only size it).
inline size_t relay_ws_layout(uint32_t n, uint32_t ntun, size_t cub_bytes, uint8_t* base, RelayWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += relay_align(std::max<size_t>(bytes, 1));
        return p;
    };
    RelayWs w{};
    w.key = (uint32_t*)take((size_t)n * 4);
    w.idx = (uint32_t*)take((size_t)n * 4);
    w.key_sorted = (uint32_t*)take((size_t)n * 4);
    w.idx_sorted = (uint32_t*)take((size_t)n * 4);
    w.rank = (uint32_t*)take((size_t)n * 4);
    w.sub_desc = (neb_desc*)take((size_t)n * sizeof(neb_desc));
    w.sub_map = (uint32_t*)take((size_t)n * 4);
    w.sub_status = (int32_t*)take((size_t)n * 4);
    w.nsub = (uint32_t*)take(4);
    w.tun_total = (uint32_t*)take((size_t)ntun * 4);
    w.cub_tmp = take(cub_bytes);
    w.cub_bytes = cub_bytes;
    if (ws) *ws = w;
    return off;
}

}  // namespace neb

// handleOutsideRelayPacket's ForwardingType branch (outside.go:220-240) for one packet of a receive
// batch, after VerifyRelay: NEB_STATUS_NOT_FORWARDED (not a verified Message/Relay packet, or the
// caller's relay lookups found no route), NEB_STATUS_BAD_KEY (no such tunnel, or it has no eKey of
// this algorithm, as the TX batch's rule) or NEB_STATUS_OK: the packet takes the
// next message counter of tunnels[route.tunnel]. h: the packet's first two bytes, read only when
// rx_status is NEB_STATUS_OK (the gate then saw at least 32 bytes). key_ok(key_id): that key is
// installed with the batch's algorithm. Shared by the host loop (window.cpp) and the plan kernels.
template <class KeyOk>
__host__ __device__ inline int32_t neb_relay_gate(int32_t rx_status, const uint8_t* h, const neb_relay_route& r,
                                                  const neb_tx_tunnel* tun, uint32_t ntun, KeyOk key_ok) {
    if (rx_status != NEB_STATUS_OK || r.tunnel == NEB_RELAY_NONE) return NEB_STATUS_NOT_FORWARDED;
    if (h[0] != 0x11u || h[1] != 1u) return NEB_STATUS_NOT_FORWARDED;  // version 1, Message, MessageRelay
    if (r.tunnel >= ntun) return NEB_STATUS_BAD_KEY;
    const uint32_t key = tun[r.tunnel].key_id;
    if (key == NEB_KEYS_MIXED || !key_ok(key)) return NEB_STATUS_BAD_KEY;
    return NEB_STATUS_OK;
}

__host__ __device__ inline uint32_t neb_relay_be32(uint32_t x) {
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

// prepareSendVia + SendVia (inside.go:442-501) for a packet that took counter c of a tunnel with
// key key_id: NEB_STATUS_EXHAUSTED (returns before Encode: nothing to write), or NEB_STATUS_OK with
// hdr = header.Encode(1, Message, MessageRelay, remote_index, c) as four little-endian dwords for
// the packet's first 16 bytes, and *d the AD-only seal over packet[:len-16] whose tag lands on the
// packet's last 16 bytes.
__host__ __device__ inline int32_t neb_relay_send_via(const neb_rx_packet& p, uint32_t remote_index, uint32_t key_id,
                                                      uint64_t c, uint32_t hdr[4], neb_desc* d) {
    if (c >= neb::kRejectAfterMessages) return NEB_STATUS_EXHAUSTED;
    const uint32_t len = p.len & ~NEB_RX_OWN_SOURCE;
    hdr[0] = 0x00000111u;
    hdr[1] = neb_relay_be32(remote_index);
    hdr[2] = neb_relay_be32((uint32_t)(c >> 32));
    hdr[3] = neb_relay_be32((uint32_t)c);
    d->src_off = d->dst_off = p.off + len - 16u;
    d->aad_off = p.off;
    d->counter = c;
    d->len = 0;
    d->aad_len = len - 16u;
    d->key_id = key_id;
    d->flags = 0;
    return NEB_STATUS_OK;
}

extern "C" size_t neb_relay_ws_bytes(uint32_t n, uint32_t ntun, size_t* cub_bytes);
// The forward half's plan on stream s, after the receive has written d_status: fwd_status, the new
// headers, the compacted seal batch (ws->sub_desc, *ws->nsub) and the tunnels' counters advanced.
extern "C" hipError_t neb_relay_plan(const neb_rx_packet* d_pk, const neb_relay_route* d_route,
                                     const int32_t* d_status, uint32_t n, neb_tx_tunnel* d_tun, uint32_t ntun,
                                     const uint32_t* d_keys, uint32_t max_keys, int alg, uint8_t* d_arena,
                                     int32_t* d_fwd_status, const neb::RelayWs* ws, hipStream_t s);
// After the seal: a forwarded packet the seal refused (its key destroyed meanwhile) gets the seal's
// status; the seal's other statuses stay in the workspace.
extern "C" hipError_t neb_relay_fix(const neb::RelayWs* ws, uint32_t n, int32_t* d_fwd_status, hipStream_t s);
