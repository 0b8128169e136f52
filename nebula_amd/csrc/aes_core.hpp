// aes_core.hpp — the T-table AES-256 core of the GCM kernels: the tables and their LDS images, the
// lookups (TLook, TLook4), the round-key sources (Rk*), the rounds and counter-mode caching.
// Included into aes_gcm.hip only (c_T0 is defined here).
#pragma once
#include "gcm_ops.hpp"

namespace neb {

// ------------------------------------------------------------------------------------------
// AES tables (FIPS-197 S-box) — T0 in little-endian column form: bytes [2S, S, S, 3S].

struct T0Table {
    uint32_t t[256];
};
constexpr uint8_t kSbox[256] = {
    0x63,0x7c,0x77,0x7b,0xf2,0x6b,0x6f,0xc5,0x30,0x01,0x67,0x2b,0xfe,0xd7,0xab,0x76,
    0xca,0x82,0xc9,0x7d,0xfa,0x59,0x47,0xf0,0xad,0xd4,0xa2,0xaf,0x9c,0xa4,0x72,0xc0,
    0xb7,0xfd,0x93,0x26,0x36,0x3f,0xf7,0xcc,0x34,0xa5,0xe5,0xf1,0x71,0xd8,0x31,0x15,
    0x04,0xc7,0x23,0xc3,0x18,0x96,0x05,0x9a,0x07,0x12,0x80,0xe2,0xeb,0x27,0xb2,0x75,
    0x09,0x83,0x2c,0x1a,0x1b,0x6e,0x5a,0xa0,0x52,0x3b,0xd6,0xb3,0x29,0xe3,0x2f,0x84,
    0x53,0xd1,0x00,0xed,0x20,0xfc,0xb1,0x5b,0x6a,0xcb,0xbe,0x39,0x4a,0x4c,0x58,0xcf,
    0xd0,0xef,0xaa,0xfb,0x43,0x4d,0x33,0x85,0x45,0xf9,0x02,0x7f,0x50,0x3c,0x9f,0xa8,
    0x51,0xa3,0x40,0x8f,0x92,0x9d,0x38,0xf5,0xbc,0xb6,0xda,0x21,0x10,0xff,0xf3,0xd2,
    0xcd,0x0c,0x13,0xec,0x5f,0x97,0x44,0x17,0xc4,0xa7,0x7e,0x3d,0x64,0x5d,0x19,0x73,
    0x60,0x81,0x4f,0xdc,0x22,0x2a,0x90,0x88,0x46,0xee,0xb8,0x14,0xde,0x5e,0x0b,0xdb,
    0xe0,0x32,0x3a,0x0a,0x49,0x06,0x24,0x5c,0xc2,0xd3,0xac,0x62,0x91,0x95,0xe4,0x79,
    0xe7,0xc8,0x37,0x6d,0x8d,0xd5,0x4e,0xa9,0x6c,0x56,0xf4,0xea,0x65,0x7a,0xae,0x08,
    0xba,0x78,0x25,0x2e,0x1c,0xa6,0xb4,0xc6,0xe8,0xdd,0x74,0x1f,0x4b,0xbd,0x8b,0x8a,
    0x70,0x3e,0xb5,0x66,0x48,0x03,0xf6,0x0e,0x61,0x35,0x57,0xb9,0x86,0xc1,0x1d,0x9e,
    0xe1,0xf8,0x98,0x11,0x69,0xd9,0x8e,0x94,0x9b,0x1e,0x87,0xe9,0xce,0x55,0x28,0xdf,
    0x8c,0xa1,0x89,0x0d,0xbf,0xe6,0x42,0x68,0x41,0x99,0x2d,0x0f,0xb0,0x54,0xbb,0x16};

constexpr uint8_t xt(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
constexpr T0Table make_t0() {
    T0Table r{};
    for (int i = 0; i < 256; i++) {
        uint32_t s = kSbox[i], s2 = xt(kSbox[i]), s3 = s2 ^ s;
        r.t[i] = s2 | (s << 8) | (s << 16) | (s3 << 24);
    }
    return r;
}
__constant__ T0Table c_T0 = make_t0();

// ------------------------------------------------------------------------------------------
// AES-256 encryption of one block per lane (little-endian column words in and out).
// ttab: LDS, 32 copies of 256 8-byte entries, entry x of copy c at byte x*256 + c*8 holding
// (T0[x], T2[x]) for c < 16 and (T2[x], T0[x]) for c >= 16, T2 = rotl16(T0). Lane l uses copy
// c = l mod 32 and reads single dwords: T0 at lb.x = 8c + 4(c >= 16), T2 at lb.y = 8c + 4(c < 16).
// A ds_read_b32 banks on (addr/4) mod 32, so the 32 lanes of a half-wave hit dwords 2c + {0,1}
// arranged to be 32 distinct banks: every lookup is conflict-free.
// high: added to both lane bases (bit 16 when the table sits at LDS byte 65536 + an offset-field
// constant, so every lookup address is still one v_perm: its byte 2 comes from the lane base)
__device__ __forceinline__ uint2 ttab_lane_base(uint32_t lane, uint32_t high = 0u) {
    const uint32_t c = lane & 31u, hi = c >> 4;
    return make_uint2((c << 3) | (hi << 2) | high, (c << 3) | ((hi ^ 1u) << 2) | high);
}
__device__ __forceinline__ uint2 ttab_entry(uint32_t i) {  // i = x*32 + c
    const uint32_t t = c_T0.t[i >> 5], t2 = __builtin_amdgcn_alignbit(t, t, 16);
    return (i & 16u) ? make_uint2(t2, t) : make_uint2(t, t2);
}

// Wave priority while a round's 16 lookups are issued (s_setprio): the SIMD arbiter then prefers
// the wave that feeds the LDS over waves busy with their XOR phase, which keeps the LDS queue
// full. Measured on C2: 0.150 -> 0.136 ms per seal launch (priority 1, 2 and 3 alike; raising it
// for the GHASH lookups as well was slower).
#ifndef NEB_PRIO
#define NEB_PRIO 3
#endif

struct RkRegs {  // wave-uniform round keys (scalar registers)
    const uint32_t* k;
    static constexpr bool kUniform = true;
    // s_setprio levels around a round's lookups (kPrioHi) and after them (kPrioLo)
    static constexpr int kPrioHi = NEB_PRIO, kPrioLo = 0;
    __device__ __forceinline__ uint4 get(int r) const {
        return make_uint4(k[4 * r], k[4 * r + 1], k[4 * r + 2], k[4 * r + 3]);
    }
};
// The same keys with the priority levels of one age rank (gcm_single_kernel: the SIMD arbiter
// prefers a SIMD's older waves at equal priority, §3.1)
template <int HI, int LO>
struct RkRegsPrio : RkRegs {
    static constexpr int kPrioHi = HI, kPrioLo = LO;
};
struct RkLds {  // per-packet round keys staged in LDS
    const uint4* base;
    static constexpr bool kUniform = false;
    static constexpr int kPrioHi = NEB_PRIO, kPrioLo = 0;
    __device__ __forceinline__ uint4 get(int r) const { return base[r]; }
};

// a ^ b ^ round-key word k: the key from a scalar register where RK's keys are wave-uniform
template <class RK>
__device__ __forceinline__ uint32_t x3k(uint32_t a, uint32_t b, uint32_t k) {
    if constexpr (RK::kUniform) return x3s(a, b, k);
    else return x3(a, b, k);
}

// T-table lookups: T0[byte k of s], T2[byte k of s] (T1 = rotl8 T0, T3 = rotl8 T2).
struct TLook {
    const uint2* ttab;
    uint2 lb;
    __device__ __forceinline__ uint32_t t0(uint32_t s, int k) const {
        return lds_at<uint32_t>(ttab, perm(s, lb.x, 0x0C020000u | ((4u + (uint32_t)k) << 8)));
    }
    __device__ __forceinline__ uint32_t t2(uint32_t s, int k) const {
        return lds_at<uint32_t>(ttab, perm(s, lb.y, 0x0C020000u | ((4u + (uint32_t)k) << 8)));
    }
    __device__ __forceinline__ uint32_t t1(uint32_t s, int k) const { return rotl8(t0(s, k)); }
    __device__ __forceinline__ uint32_t t3(uint32_t s, int k) const { return rotl8(t2(s, k)); }
    // the round's row-1/row-3 lookups before their rotation (one rotate per column, below)
    __device__ __forceinline__ uint32_t t1r(uint32_t s, int k) const { return t0(s, k); }
    __device__ __forceinline__ uint32_t t3r(uint32_t s, int k) const { return t2(s, k); }
    static constexpr bool kFour = false;
};

// Four T-tables (T0..T3) in LDS, 128 KiB: region A (byte offset 0) holds the pairs (T0[x], T1[x]),
// region B (offset 64 KiB) the pairs (T2[x], T3[x]), each laid out and swizzled like TLook's
// (32 copies, copy c of entry x at x*256 + c*8, the two dwords swapped for c >= 16). A round then
// combines each column with two XOR3s and no rotates (8 VALU per round fewer than TLook), at
// the price of one 1024-lane workgroup per CU. One lane base serves all four tables: byte 0 =
// the lane's row-0/row-2 dword offset in its 256-byte row, byte 3 = its row-1/row-3 dword offset,
// byte 2 = 1 (region B); each lookup's v_perm picks byte 0 or 3 and zero or byte 2.
__device__ __forceinline__ uint32_t ttab4_lane_base(uint32_t lane) {
    const uint32_t c = lane & 31u, hi = c >> 4;
    return ((c << 3) | (hi << 2)) | (1u << 16) | (((c << 3) | ((hi ^ 1u) << 2)) << 24);
}
__device__ __forceinline__ uint2 ttab4_entry(uint32_t i) {  // i = region*8192 + x*32 + c
    uint32_t t = c_T0.t[(i >> 5) & 255u];
    if (i & 8192u) t = __builtin_amdgcn_alignbit(t, t, 16);  // T2 = rotl16 T0
    const uint32_t t1 = rotl8(t);                            // T1 = rotl8 T0, T3 = rotl8 T2
    return (i & 16u) ? make_uint2(t1, t) : make_uint2(t, t1);
}
// Write N entries of an LDS T-table image with THREADS threads: every source word is loaded
// before any is stored, so the prologue pays one global-load latency instead of one per entry (a
// strided loop left a load + vmcnt(0) + store per iteration: 16 serialised L2 round trips).
template <uint32_t N, uint32_t THREADS, class F>
__device__ __forceinline__ void fill_ttab(uint2* dst, uint32_t tid, F entry) {
    constexpr uint32_t K = (N + THREADS - 1) / THREADS;
    constexpr bool kWhole = N % THREADS == 0;
    uint2 v[K];
#pragma unroll
    for (uint32_t j = 0; j < K; j++) v[j] = entry((tid + j * THREADS) % N);
#pragma unroll
    for (uint32_t j = 0; j < K; j++)
        if (kWhole || tid + j * THREADS < N) dst[tid + j * THREADS] = v[j];
}
struct TLook4 {
    const uint2* ttab;
    uint32_t lb;
    __device__ __forceinline__ uint32_t at(uint32_t s, int k, uint32_t sel) const {
        return lds_at<uint32_t>(ttab, perm(s, lb, sel | ((4u + (uint32_t)k) << 8)));
    }
    __device__ __forceinline__ uint32_t t0(uint32_t s, int k) const { return at(s, k, 0x0C0C0000u); }
    __device__ __forceinline__ uint32_t t1(uint32_t s, int k) const { return at(s, k, 0x0C0C0003u); }
    __device__ __forceinline__ uint32_t t2(uint32_t s, int k) const { return at(s, k, 0x0C020000u); }
    __device__ __forceinline__ uint32_t t3(uint32_t s, int k) const { return at(s, k, 0x0C020003u); }
    __device__ __forceinline__ uint32_t t1r(uint32_t s, int k) const { return t1(s, k); }
    __device__ __forceinline__ uint32_t t3r(uint32_t s, int k) const { return t3(s, k); }
    static constexpr bool kFour = true;
};

// AES-256 rounds FIRST..13 (full) and 14 (final) on the state s0..s3 (after round FIRST-1).
template <int FIRST, class TL, class RK>
__device__ __forceinline__ uint4 aes256_rounds(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, const TL& T,
                                               const RK& rk) {
    uint4 k;
#pragma unroll
    for (int r = FIRST; r < 14; r++) {
        k = rk.get(r);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(RK::kPrioHi);
        const uint32_t a0 = T.t0(s0, 0), a1 = T.t1r(s1, 1), a2 = T.t2(s2, 2), a3 = T.t3r(s3, 3);
        const uint32_t b0 = T.t0(s1, 0), b1 = T.t1r(s2, 1), b2 = T.t2(s3, 2), b3 = T.t3r(s0, 3);
        const uint32_t c0 = T.t0(s2, 0), c1 = T.t1r(s3, 1), c2 = T.t2(s0, 2), c3 = T.t3r(s1, 3);
        const uint32_t d0 = T.t0(s3, 0), d1 = T.t1r(s0, 1), d2 = T.t2(s1, 2), d3 = T.t3r(s2, 3);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(RK::kPrioLo);
        // T0[a] ^ T1[b] ^ T2[c] ^ T3[d] ^ k; with two tables T1 = rotl8 T0, T3 = rotl8 T2
        if constexpr (TL::kFour) {
            s0 = x3k<RK>(x3(a0, a1, a2), a3, k.x);
            s1 = x3k<RK>(x3(b0, b1, b2), b3, k.y);
            s2 = x3k<RK>(x3(c0, c1, c2), c3, k.z);
            s3 = x3k<RK>(x3(d0, d1, d2), d3, k.w);
        } else {
            s0 = x3k<RK>(a0, a2, k.x) ^ rotl8(a1 ^ a3);
            s1 = x3k<RK>(b0, b2, k.y) ^ rotl8(b1 ^ b3);
            s2 = x3k<RK>(c0, c2, k.z) ^ rotl8(c1 ^ c3);
            s3 = x3k<RK>(d0, d2, k.w) ^ rotl8(d1 ^ d3);
        }
    }
    k = rk.get(14);
    // last round: SubBytes+ShiftRows; S[x] is byte 1 of T0[x]
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(RK::kPrioHi);
    const uint32_t a0 = T.t0(s0, 0), a1 = T.t0(s1, 1), a2 = T.t0(s2, 2), a3 = T.t0(s3, 3);
    const uint32_t b0 = T.t0(s1, 0), b1 = T.t0(s2, 1), b2 = T.t0(s3, 2), b3 = T.t0(s0, 3);
    const uint32_t c0 = T.t0(s2, 0), c1 = T.t0(s3, 1), c2 = T.t0(s0, 2), c3 = T.t0(s1, 3);
    const uint32_t d0 = T.t0(s3, 0), d1 = T.t0(s0, 1), d2 = T.t0(s1, 2), d3 = T.t0(s2, 3);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(RK::kPrioLo);
    uint4 o;
    o.x = x3k<RK>(perm(a1, a0, 0x0C0C0501u), perm(a3, a2, 0x05010C0Cu), k.x);
    o.y = x3k<RK>(perm(b1, b0, 0x0C0C0501u), perm(b3, b2, 0x05010C0Cu), k.y);
    o.z = x3k<RK>(perm(c1, c0, 0x0C0C0501u), perm(c3, c2, 0x05010C0Cu), k.z);
    o.w = x3k<RK>(perm(d1, d0, 0x0C0C0501u), perm(d3, d2, 0x05010C0Cu), k.w);
    return o;
}

template <class TL, class RK>
__device__ __forceinline__ uint4 aes256_block(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, const TL& T,
                                              const RK& rk) {
    const uint4 k = rk.get(0);
    return aes256_rounds<1>(s0 ^ k.x, s1 ^ k.y, s2 ^ k.z, s3 ^ k.w, T, rk);
}

// Counter-mode caching. A packet's counter blocks are 00000000 || BE64(n) || BE32(ctr): with
// ctr < 2^16 they differ only in state bytes 14 and 15 (word 3, bytes 2 and 3). Round 1 then
// varies only through T2[byte 14] in column 1 and T3[byte 15] in column 0, and round 2 only
// through the two varying columns of round 1: per block 2 + 8 lookups instead of 32. K (round 1)
// and L (round 2) hold the packet-constant parts, round keys folded in.
struct CtrConst {
    uint4 K, L;
    uint32_t k0w;  // word 3 of round key 0
};

template <class TL, class RK>
__device__ __forceinline__ CtrConst aes_ctr_prep(uint32_t c1, uint32_t c2, const TL& T, const RK& rk) {
    const uint4 k0 = rk.get(0), k1 = rk.get(1), k2 = rk.get(2);
    const uint32_t s0 = k0.x, s1 = c1 ^ k0.y, s2 = c2 ^ k0.z, s3 = k0.w;  // counter bytes = 0
    CtrConst c;
    c.k0w = k0.w;
    c.K.x = T.t0(s0, 0) ^ rotl8(T.t0(s1, 1)) ^ T.t2(s2, 2) ^ k1.x;                      // minus T3[b3 s3]
    c.K.y = T.t0(s1, 0) ^ rotl8(T.t0(s2, 1)) ^ rotl8(T.t2(s0, 3)) ^ k1.y;               // minus T2[b2 s3]
    c.K.z = T.t0(s2, 0) ^ rotl8(T.t0(s3, 1) ^ T.t2(s1, 3)) ^ T.t2(s0, 2) ^ k1.z;
    c.K.w = T.t0(s3, 0) ^ rotl8(T.t0(s0, 1) ^ T.t2(s2, 3)) ^ T.t2(s1, 2) ^ k1.w;
    c.L.x = T.t2(c.K.z, 2) ^ rotl8(T.t2(c.K.w, 3)) ^ k2.x;
    c.L.y = rotl8(T.t0(c.K.z, 1)) ^ T.t2(c.K.w, 2) ^ k2.y;
    c.L.z = T.t0(c.K.z, 0) ^ rotl8(T.t0(c.K.w, 1)) ^ k2.z;
    c.L.w = T.t0(c.K.w, 0) ^ rotl8(T.t2(c.K.z, 3)) ^ k2.w;
    return c;
}

template <class TL, class RK>
__device__ __forceinline__ uint4 aes256_ctr_block(const CtrConst& c, uint32_t ctr, const TL& T, const RK& rk) {
    const uint32_t s3 = c.k0w ^ bswap32(ctr);
    const uint32_t t0 = c.K.x ^ T.t3(s3, 3);
    const uint32_t t1 = c.K.y ^ T.t2(s3, 2);
    const uint32_t u0 = x3(c.L.x, T.t0(t0, 0), T.t1(t1, 1));
    const uint32_t u1 = x3(c.L.y, T.t0(t1, 0), T.t3(t0, 3));
    const uint32_t u2 = x3(c.L.z, T.t2(t0, 2), T.t3(t1, 3));
    const uint32_t u3 = x3(c.L.w, T.t2(t1, 2), T.t1(t0, 1));
    return aes256_rounds<3>(u0, u1, u2, u3, T, rk);
}

// The same with every counter below 2^8 (packets under 4 KiB): byte 14 is zero too, so round 1
// varies only through T3[byte 15] in column 0, and round 2 through the 4 bytes of that column,
// one per output column: 1 + 4 lookups per block instead of 2 + 8.
template <class TL, class RK>
__device__ __forceinline__ CtrConst aes_ctr_prep8(uint32_t c1, uint32_t c2, const TL& T, const RK& rk) {
    CtrConst c = aes_ctr_prep(c1, c2, T, rk);
    const uint4 k2 = rk.get(2);
    c.K.y ^= T.t2(c.k0w, 2);  // round 1 column 1 is constant now
    c.L.x = rotl8(T.t0(c.K.y, 1)) ^ T.t2(c.K.z, 2) ^ rotl8(T.t2(c.K.w, 3)) ^ k2.x;
    c.L.y = T.t0(c.K.y, 0) ^ rotl8(T.t0(c.K.z, 1)) ^ T.t2(c.K.w, 2) ^ k2.y;
    c.L.z = T.t0(c.K.z, 0) ^ rotl8(T.t0(c.K.w, 1) ^ T.t2(c.K.y, 3)) ^ k2.z;
    c.L.w = T.t0(c.K.w, 0) ^ T.t2(c.K.y, 2) ^ rotl8(T.t2(c.K.z, 3)) ^ k2.w;
    return c;
}

template <class TL, class RK>
__device__ __forceinline__ uint4 aes256_ctr8_block(const CtrConst& c, uint32_t ctr, const TL& T, const RK& rk) {
    const uint32_t t0 = c.K.x ^ T.t3(c.k0w ^ (ctr << 24), 3);
    const uint32_t u0 = c.L.x ^ T.t0(t0, 0);
    const uint32_t u1 = c.L.y ^ T.t3(t0, 3);
    const uint32_t u2 = c.L.z ^ T.t2(t0, 2);
    const uint32_t u3 = c.L.w ^ T.t1(t0, 1);
    return aes256_rounds<3>(u0, u1, u2, u3, T, rk);
}

}  // namespace neb
