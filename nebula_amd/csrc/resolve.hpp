// resolve.hpp — the device half of the index table (resolve.hip), shared with index.cpp: the
// scatter that applies an update to a device image, and the resolve kernel's launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "index_core.hpp"

namespace neb {

// One slot's new state, in pinned host memory the scatter kernel reads directly.
struct IdxOp {
    uint64_t slot;
    uint64_t tag;  // kIdxTomb: tombstone the slot; else publish {a, b} and then this tag
    uint64_t a, b;
};

}  // namespace neb

// ops[0..n) applied to `image` on s, one thread each (every op names another slot). A record is
// written and released before its tag is published. The order of the launches is table_mirror.hpp's.
extern "C" hipError_t neb_idx_scatter(neb::IdxSlot* image, const neb::IdxOp* ops, uint32_t n, hipStream_t s);
// neb_rx_resolve_batch's kernel on s over `image` (mask + 1 slots). nets travels by value.
extern "C" hipError_t neb_idx_resolve(const neb::IdxSlot* image, uint32_t mask, const neb::IdxNets* nets,
                                      neb_rx_packet* d_pk, const neb_rx_source* d_src, uint32_t n,
                                      const uint8_t* d_arena, neb_relay_route* d_route, neb_rx_via* d_via,
                                      hipStream_t s);
