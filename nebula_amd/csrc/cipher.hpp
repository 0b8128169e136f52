// cipher.hpp — the host launchers of the AEAD kernels (aes_gcm.hip, chacha_poly.hip) that engine.cpp
// calls, described at their definitions, and the sizes both sides of the per-packet path agree on.
// The defining files include it too, so the compiler checks each definition against its declaration.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "host_common.hpp"  // kOneBytes, kCombMax, kCombSlot

extern "C" {
hipError_t neb_gcm_probe(void);
// n keys (32 B each, mapped host memory) into the records of key slots slots[0..n): one launch
hipError_t neb_gcm_key_setup(const uint8_t* keys, const uint32_t* slots, uint32_t n, uint32_t* table, hipStream_t s);
hipError_t neb_chacha_key_setup(const uint8_t* keys, const uint32_t* slots, uint32_t n, uint32_t* table, hipStream_t s);
hipError_t neb_gcm_batch_single(int open, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena, const uint32_t* d_keys,
                                uint32_t max_keys, uint32_t key_hint, int32_t* d_status, const uint32_t* d_n,
                                int cu_count, hipStream_t s, int hdr_from_dst, hipEvent_t stop, const uint8_t* rx);
hipError_t neb_chacha_batch(int open, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena, const uint32_t* d_keys,
                            uint32_t max_keys, uint32_t key_hint, int32_t* d_status, const uint32_t* d_n, int cu_count,
                            hipStream_t s, int hdr_from_dst, hipEvent_t stop, const uint8_t* rx);
hipError_t neb_gcm_batch_chunked(int open, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena, const uint32_t* d_keys,
                                 uint32_t max_keys, int32_t* d_status, const uint32_t* d_sorted, const uint4* d_chunks,
                                 uint32_t* d_counters, uint32_t max_chunks, int cu_count, hipStream_t s,
                                 int hdr_from_dst, hipEvent_t stop, const uint8_t* rx);
uint32_t neb_gcm_single_slots(uint32_t n, int cu_count, int open, int hdr_from_dst);
hipError_t neb_gcm_one(int open, const uint8_t* aad, uint32_t aad_len, const uint8_t* in, uint32_t in_len, uint32_t len,
                       uint64_t counter, uint8_t* out, int32_t* status, const uint32_t* d_keys, uint32_t max_keys,
                       uint32_t key, hipStream_t s);
hipError_t neb_chacha_one(int open, const uint8_t* aad, uint32_t aad_len, const uint8_t* in, uint32_t in_len,
                          uint32_t len, uint64_t counter, uint8_t* out, int32_t* status, const uint32_t* d_keys,
                          uint32_t max_keys, uint32_t key, hipStream_t s);
hipError_t neb_gcm_one_batch(int open, const neb_desc* descs, int32_t* status, uint8_t* slots, uint32_t n,
                             const uint32_t* d_keys, uint32_t max_keys, hipStream_t s);
hipError_t neb_copy_desc(neb_desc* dst, const neb_desc* src, uint32_t n, hipStream_t s);
}
