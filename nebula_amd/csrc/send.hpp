// send.hpp — device workspace of the TX send plan (send.hip), shared with engine.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "send_core.hpp"

namespace neb {

struct SendPrev {   // the scan element of the first pass
    uint32_t last;  // 1 + the last wire so far that is not absent (0: none): max
    uint32_t rank;  // routable wires so far: sum
};

// All by wire index.
struct SendWs {
    SendRec* rec;      // class, destination, length
    SendPrev* p_in;    // this wire's own contribution
    SendPrev* p_out;   // exclusive scan: the previous wire that is not absent, the routable rank
    uint32_t* flags;   // kSendFlag*
    uint32_t* ps_in;   // a plateau's first wire: its rank; else 0
    uint32_t* ps_out;  // inclusive max: the rank at which this wire's plateau starts
    uint32_t* fn_in;   // a plateau's first wire: the plateau before it as a function; else the identity
    uint32_t* fn_out;  // inclusive scan under composition: bit 0 = this wire's plateau's o
    uint32_t* st_in;   // 1: this wire starts a run
    uint32_t* st_out;  // inclusive sum: 1 + this wire's entry
    uint32_t* efirst;  // by entry: the rank of its first wire
    uint32_t* edst;    // by entry: its destination tunnel
    void* cub_tmp;
    size_t cub_bytes;
};

inline size_t send_ws_layout(uint32_t n, size_t cub_bytes, uint8_t* base, SendWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const size_t m = n ? n : 1;
    SendWs w{};
    w.rec = (SendRec*)take(m * sizeof(SendRec));
    w.p_in = (SendPrev*)take(m * sizeof(SendPrev));
    w.p_out = (SendPrev*)take(m * sizeof(SendPrev));
    w.flags = (uint32_t*)take(m * 4);
    w.ps_in = (uint32_t*)take(m * 4);
    w.ps_out = (uint32_t*)take(m * 4);
    w.fn_in = (uint32_t*)take(m * 4);
    w.fn_out = (uint32_t*)take(m * 4);
    w.st_in = (uint32_t*)take(m * 4);
    w.st_out = (uint32_t*)take(m * 4);
    w.efirst = (uint32_t*)take(m * 4);
    w.edst = (uint32_t*)take(m * 4);
    w.cub_tmp = take(cub_bytes);
    w.cub_bytes = cub_bytes;
    if (ws) *ws = w;
    return off;
}

struct SendArgs {
    const neb_tx_wire* wires;
    const int32_t* wire_status;
    const uint32_t* nwires;
    const neb_tx_packet* packets;
    const neb_relay_route* via;
    const neb_udp_addr* remote;
    neb_send_iov* iov;
    uint32_t* niov;
    neb_send_entry* entries;
    uint32_t* nentries;
    uint32_t* wire_entry;
    int32_t* send_status;
    uint32_t n, npackets, ntunnels, socket_v4, max_segments, chunk_packets;
    SendWs ws;
};

}  // namespace neb

extern "C" size_t neb_send_ws_bytes(uint32_t n, size_t* cub_bytes);
// Enqueues the whole plan of a.n >= 1 wire slots on s (a.ws: a workspace laid out for at least a.n).
extern "C" hipError_t neb_send_run(const neb::SendArgs* a, hipStream_t s);
