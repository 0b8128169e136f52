// coalesce.hpp — device workspace of the receive coalescer (coalesce.hip), shared with engine.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "coalesce_core.hpp"

namespace neb {

struct Co3 {  // slots created per lane (TCP, UDP, passthrough): the scan element of the emission order
    uint32_t a[3];
};
struct CoCopy {  // one packet's bytes in the output: the gather kernel's work item
    uint64_t src_off;
    uint64_t dst_off;
    uint32_t len;  // 0: nothing to copy
    uint32_t pad;
};

// "pos" is a packet's position in (epoch, counter) order: time, for every rule of the lanes.
struct CoWs {
    CoRec* rec;        // by input index: class, lane, lane parse
    uint32_t* hash;    // by input index: flow hash
    uint64_t* k0;      // sort keys / scan inputs, reused stage by stage
    uint64_t* k1;
    uint32_t* i0;      // sort values
    uint32_t* i1;
    uint32_t* order;   // pos -> input index
    uint64_t* bar;     // by pos: unparseable packets so far, TCP lane << 32 | UDP lane (inclusive)
    uint32_t* fpos;    // flow order -> pos
    uint32_t* fprev;   // by pos: the flow's previous data / sealing packet, kCoNone
    uint32_t* fnext;
    uint32_t* lw;      // by pos: pay_len | PSH << 17 | link << 18 | data << 19
    uint32_t* jump0;   // by pos: next seed if this packet were one (pointer jumping, ping-pong)
    uint32_t* jump1;
    uint32_t* reach;   // by pos: 1 = a data packet that is a seed
    uint32_t* cnseg;   // by pos: the chain seeded here: segments
    uint32_t* ctotal;  //          payload bytes | PSH of an appended segment << 31
    uint32_t* mseed;   // by pos: the seed of the chain this data packet rides (pos)
    uint32_t* midx;    //          and its segment index
    Co3* sc_in;        // by pos: slot created here, per lane
    Co3* sc_out;       // exclusive scan
    uint32_t* wk;      // by pos: the write of the slot created here
    uint64_t* wsize;   // by write: 16-aligned bytes
    uint64_t* woff;    // exclusive scan
    uint32_t* wpos;    // by write: the pos that created it
    CoCopy* cp;        // by pos
    void* cub_tmp;
    size_t cub_bytes;
};

inline size_t co_ws_align(size_t x) { return (x + 255) & ~(size_t)255; }

// Carve a CoWs out of `base` (nullptr: only size it). Returns the bytes needed.
inline size_t co_ws_layout(uint32_t n, size_t cub_bytes, uint8_t* base, CoWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += co_ws_align(bytes);
        return p;
    };
    const size_t m = n ? n : 1;
    CoWs w{};
    w.rec = (CoRec*)take(m * sizeof(CoRec));
    w.hash = (uint32_t*)take(m * 4);
    w.k0 = (uint64_t*)take(m * 8);
    w.k1 = (uint64_t*)take(m * 8);
    w.i0 = (uint32_t*)take(m * 4);
    w.i1 = (uint32_t*)take(m * 4);
    w.order = (uint32_t*)take(m * 4);
    w.bar = (uint64_t*)take(m * 8);
    w.fpos = (uint32_t*)take(m * 4);
    w.fprev = (uint32_t*)take(m * 4);
    w.fnext = (uint32_t*)take(m * 4);
    w.lw = (uint32_t*)take(m * 4);
    w.jump0 = (uint32_t*)take(m * 4);
    w.jump1 = (uint32_t*)take(m * 4);
    w.reach = (uint32_t*)take(m * 4);
    w.cnseg = (uint32_t*)take(m * 4);
    w.ctotal = (uint32_t*)take(m * 4);
    w.mseed = (uint32_t*)take(m * 4);
    w.midx = (uint32_t*)take(m * 4);
    w.sc_in = (Co3*)take(m * sizeof(Co3));
    w.sc_out = (Co3*)take(m * sizeof(Co3));
    w.wk = (uint32_t*)take(m * 4);
    w.wsize = (uint64_t*)take(m * 8);
    w.woff = (uint64_t*)take(m * 8);
    w.wpos = (uint32_t*)take(m * 4);
    w.cp = (CoCopy*)take(m * sizeof(CoCopy));
    w.cub_tmp = take(cub_bytes);
    w.cub_bytes = cub_bytes;
    if (ws) *ws = w;
    return off;
}

}  // namespace neb

extern "C" size_t neb_co_ws_bytes(uint32_t n, size_t* cub_bytes);
// Enqueues the whole coalesce of n >= 1 records on s. hash_bits: the bits of the flow hash kept.
extern "C" hipError_t neb_co_run(const neb_plain_packet* d_plain, uint32_t n, const uint8_t* d_in, uint8_t* d_out,
                                 uint64_t out_cap, neb_tun_write* d_writes, uint32_t max_writes, uint32_t* d_nwrites,
                                 uint32_t* d_pkt_write, int32_t* d_pkt_status, uint32_t lanes, uint32_t hash_bits,
                                 const neb::CoWs* ws, hipStream_t s);
extern "C" hipError_t neb_co_plain_from_wire(const neb_rx_packet* d_pk, const int32_t* d_status,
                                             const uint64_t* d_epoch, uint32_t nepoch, uint32_t n,
                                             const uint8_t* d_arena, neb_plain_packet* d_plain, hipStream_t s);
