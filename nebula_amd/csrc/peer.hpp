// peer.hpp — the device half of the peer table (peer.hip), shared with peer.cpp: the inner resolve
// kernel's launch. The table's images are written by the TX table's scatter (route.hpp): the slots
// are the same.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "peer_core.hpp"

// neb_rx_inner_batch's kernel on s over `image` (mask + 1 slots). lens and routable travel by value.
extern "C" hipError_t neb_peer_inner(const neb::TxSlot* image, uint32_t mask, const neb::TxLens* lens,
                                     const neb::PeerRoutable* routable, const neb_rx_packet* d_pk,
                                     const int32_t* d_status, const uint64_t* d_epoch, uint32_t nepoch, uint32_t n,
                                     const uint8_t* d_arena, neb_plain_packet* d_plain, neb_fw_packet* d_fw,
                                     int32_t* d_inner_status, hipStream_t s);
