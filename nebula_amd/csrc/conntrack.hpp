// conntrack.hpp — the device workspace and the launchers of the connection table (conntrack.hip),
// shared with conntrack.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "conntrack_core.hpp"

namespace neb {

// The lookup's workspace, laid out for max_batch packets at create.
struct CtWs {
    uint32_t* flag;  // by packet: 1 goes to the host's work list
    uint32_t* pos;   // the exclusive sum of flag
    uint64_t* acc;   // {hits, misses, stales}: zero between calls (the scatter hands them over)
    void* cub_tmp;
    size_t cub_bytes;
};

inline size_t ct_ws_layout(uint32_t n, size_t cub_bytes, uint8_t* base, CtWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const size_t m = n ? n : 1;
    CtWs w{};
    w.acc = (uint64_t*)take(32);
    w.flag = (uint32_t*)take(m * 4);
    w.pos = (uint32_t*)take(m * 4);
    w.cub_tmp = take(cub_bytes);
    w.cub_bytes = cub_bytes;
    if (ws) *ws = w;
    return off;
}

struct CtLookupArgs {
    CtSlot* slots;
    const neb_fw_packet* fw;
    int32_t* status;
    uint8_t* verdict;
    neb_plain_packet* plain;
    neb_tx_packet* tx;
    neb_ct_work* work;
    uint32_t* counts;
    uint64_t now;
    CtParams p;
    uint32_t n, version, work_cap;
    CtWs ws;
};

struct CtAddArgs {
    CtSlot* slots;
    uint64_t* counters;  // {live, tombstones}
    const neb_fw_packet* keys;
    const uint8_t* incoming;
    neb_ct_result* result;
    uint64_t now;
    CtParams p;
    uint32_t n, version;
};

struct CtEvictArgs {
    CtSlot* slots;
    uint64_t* counters;
    const neb_fw_packet* keys;
    int64_t* remaining;
    uint64_t now;
    CtParams p;
    uint32_t n, force;
};

}  // namespace neb

extern "C" size_t neb_ct_ws_bytes(uint32_t n, size_t* cub_bytes);
// Each enqueues its launches on s (n != 0).
extern "C" hipError_t neb_ct_lookup(const neb::CtLookupArgs* a, hipStream_t s);
extern "C" hipError_t neb_ct_add(const neb::CtAddArgs* a, hipStream_t s);
extern "C" hipError_t neb_ct_evict(const neb::CtEvictArgs* a, hipStream_t s);
// Every settled slot of `from` into the cleared image `to` (the same parameters), and tombstones = 0.
extern "C" hipError_t neb_ct_rehash(const neb::CtSlot* from, neb::CtSlot* to, uint64_t* counters, const neb::CtParams* p,
                                    hipStream_t s);
