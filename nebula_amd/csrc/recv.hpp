// recv.hpp — device workspace of the RX receive plan (recv.hip), shared with engine.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "recv_core.hpp"

namespace neb {

// All by entry index.
struct RecvWs {
    uint64_t* cnt;    // the entry's packets
    uint64_t* first;  // exclusive sum: the packets before it
    int32_t* seg;     // its segment size (the cmsg walk's, or the caller's)
    void* cub_tmp;
    size_t cub_bytes;
};

inline size_t recv_ws_layout(uint32_t n, size_t cub_bytes, uint8_t* base, RecvWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const size_t m = n ? n : 1;
    RecvWs w{};
    w.cnt = (uint64_t*)take(m * 8);
    w.first = (uint64_t*)take(m * 8);
    w.seg = (int32_t*)take(m * 4);
    w.cub_tmp = take(cub_bytes);
    w.cub_bytes = cub_bytes;
    if (ws) *ws = w;
    return off;
}

struct RecvArgs {
    const neb_recv_entry* entries;
    const uint8_t* ctrl;
    neb_rx_packet* pk;
    neb_rx_source* src;
    uint32_t* pkt_entry;
    neb_udp_addr* from;
    uint32_t* entry_first;
    uint32_t* counts;
    uint32_t n, max_packets, ctrl_stride, socket_v4;
    RecvWs ws;
};

}  // namespace neb

extern "C" size_t neb_recv_ws_bytes(uint32_t n, size_t* cub_bytes);
// Enqueues the whole plan on s (a.ws: a workspace laid out for at least a.n entries). a.n and
// a.max_packets may each be 0.
extern "C" hipError_t neb_recv_run(const neb::RecvArgs* a, hipStream_t s);
