// route.hpp — the device half of the TX table (route.hip), shared with route.cpp: the scatter that
// applies a host update to a device image, and the resolve kernel's launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "route_core.hpp"

namespace neb {

// One slot's new state, in pinned host memory the scatter kernel reads directly.
struct TxOp {
    uint64_t slot;
    uint64_t tag;  // kTxTomb: tombstone the slot; else publish {addr_lo, addr_hi, value} and then this tag
    uint64_t addr_lo, addr_hi, value;
};

}  // namespace neb

// ops[0..n) applied to `image` (mask + 1 slots) on s, one thread each (every op names another
// slot). A record is written and released before its tag is published.
extern "C" hipError_t neb_txt_scatter(neb::TxSlot* image, uint32_t mask, const neb::TxOp* ops, uint32_t n, hipStream_t s);
// neb_tx_resolve_batch's kernel on s over `image` (mask + 1 slots) and its gateway array. lens and
// own travel by value.
extern "C" hipError_t neb_txt_resolve(const neb::TxSlot* image, uint32_t mask, const neb::TxGw* gws,
                                      const neb::TxLens* lens, const neb::TxOwn* own, neb_tx_packet* d_pk, uint32_t n,
                                      const uint8_t* d_in, neb_fw_packet* d_fw, int32_t* d_status, hipStream_t s);
