// gcm_ops.hpp — one-instruction helpers and LDS reads shared by the AES core, the GF(2^128)
// arithmetic and the packet group (included into aes_gcm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace neb {

// Three-input XOR in one VALU op. gfx950 has no v_xor3_b32; its v_bitop3_b32 evaluates any
// 3-input truth table (0x96 = a ^ b ^ c), but hipcc does not form it from a ^ b ^ c chains.
__device__ __forceinline__ uint32_t x3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// same, third operand wave-uniform (a round key in an SGPR)
__device__ __forceinline__ uint32_t x3s(uint32_t a, uint32_t b, uint32_t k) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "s"(k));
    return r;
}
__device__ __forceinline__ uint32_t rotl8(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 24); }
__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint4 sel4(bool c, uint4 a, uint4 b) {
    return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
__device__ __forceinline__ uint4 bswap4(uint4 v) { return make_uint4(bswap32(v.x), bswap32(v.y), bswap32(v.z), bswap32(v.w)); }
__device__ __forceinline__ uint4 shfl_xor4(uint4 v, int m) {
    return make_uint4(__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m), __shfl_xor(v.w, m));
}
__device__ __forceinline__ uint4 shfl4(uint4 v, uint32_t src) {
    return make_uint4(__shfl(v.x, (int)src), __shfl(v.y, (int)src), __shfl(v.z, (int)src), __shfl(v.w, (int)src));
}

template <class T>
__device__ __forceinline__ T lds_at(const void* base, uint32_t byte_off) {
    // every table offset is a multiple of sizeof(T): say so, or 16-byte reads get split into
    // ds_read2/b96 pieces that conflict
    return *reinterpret_cast<const T*>(
        __builtin_assume_aligned(reinterpret_cast<const char*>(base) + byte_off, sizeof(T)));
}

// One ds_read_b64. The load is volatile so that two of them off one address register stay two
// instructions: merged into a ds_read2_b64 they would bank on (addr/4) mod 32 and cost 8 LDS cycles
// instead of 2 + 2.
__device__ __forceinline__ uint2 lds_b64(const void* base, uint32_t byte_off) {
    typedef uint32_t v2u __attribute__((ext_vector_type(2)));
    // (the LDS address space is named: a volatile access through a generic pointer stays a flat load)
    typedef const volatile __attribute__((address_space(3))) v2u* lds_ptr;
    const v2u v = *(lds_ptr)__builtin_assume_aligned(reinterpret_cast<const char*>(base) + byte_off, 8);
    return make_uint2(v.x, v.y);
}

}  // namespace neb
