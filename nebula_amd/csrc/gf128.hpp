// gf128.hpp — GF(2^128) in GCM bit order for the GHASH of the GCM kernels: shifts and the reduction,
// the table multiplies (5-bit windows, position tables, Shoup tables) and table entries.
#pragma once
#include "gcm_ops.hpp"

namespace neb {

// ------------------------------------------------------------------------------------------
// GF(2^128), GCM bit order. An element is 4 big-endian words w0..w3; the coefficient of x^j is
// bit 31 - (j mod 32) of w[j / 32], so multiplying by x is a 128-bit logical right shift.
// Nibble p (p = 8q + r, 0..31) of x = bits 28-4r..31-4r of w[q]; its value v has MSB = x^(4p).

__device__ __forceinline__ uint4 gf_mulx(uint4 v) {
    uint32_t lsb = v.w & 1u;
    uint4 r;
    r.w = shr64(v.z, v.w, 1);
    r.z = shr64(v.y, v.z, 1);
    r.y = shr64(v.x, v.y, 1);
    r.x = (v.x >> 1) ^ (lsb ? 0xE1000000u : 0u);
    return r;
}

// 256-bit product z[0..7] (x^0..x^255) -> 128-bit, modulo x^128 + x^7 + x^2 + x + 1.
__device__ __forceinline__ uint4 gf_reduce(const uint32_t z[8]) {
    const uint32_t l0 = z[4], l1 = z[5], l2 = z[6], l3 = z[7];
    // L·(1 + x + x^2 + x^7), the bits shifted out (x^128..x^134) collected in o
    uint32_t t0 = x3(l0, l0 >> 1, l0 >> 2) ^ (l0 >> 7);
    uint32_t t1 = x3(x3(l1, shr64(l0, l1, 1), shr64(l0, l1, 2)), shr64(l0, l1, 7), z[1]);
    uint32_t t2 = x3(x3(l2, shr64(l1, l2, 1), shr64(l1, l2, 2)), shr64(l1, l2, 7), z[2]);
    uint32_t t3 = x3(x3(l3, shr64(l2, l3, 1), shr64(l2, l3, 2)), shr64(l2, l3, 7), z[3]);
    uint32_t o = x3(l3 << 31, l3 << 30, l3 << 25);
    uint32_t of = x3(o, o >> 1, o >> 2) ^ (o >> 7);
    return make_uint4(x3(z[0], t0, of), t1, t2, t3);
}

// q·x^i, i < 128: q shifted right by i bits as a 256-bit product, then reduced (any lane, no loop).
__device__ __forceinline__ uint4 gf_mul_xpow(uint4 q, uint32_t i) {
    const uint32_t w = i >> 5, b = i & 31u;
    const uint32_t src[4] = {q.x, q.y, q.z, q.w};
    uint32_t y[8], z[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) v = (uint32_t)(k - j) == w ? src[j] : v;
        y[k] = v;
    }
    z[0] = y[0] >> b;
#pragma unroll
    for (int k = 1; k < 8; k++) z[k] = shr64(y[k - 1], y[k], b);
    return gf_reduce(z);
}

// q·x^b, b < 32 (gf_mul_xpow with no whole-word shift): 128 + 32 bits, the top word reduced.
__device__ __forceinline__ uint4 gf_mul_xpow32(uint4 q, uint32_t b) {
    const uint32_t z[8] = {q.x >> b, shr64(q.x, q.y, b), shr64(q.y, q.z, b), shr64(q.z, q.w, b), shr64(q.w, 0u, b),
                           0u, 0u, 0u};
    return gf_reduce(z);
}

// (byte K of w) & 0xF0 in one VALU op (SDWA byte select); hipcc emits a shift + and for most K.
template <int K>
__device__ __forceinline__ uint32_t byte_hi_nibble(uint32_t w) {
    uint32_t r;
    if constexpr (K == 0) {
        r = w & 0xF0u;
    } else {
        asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_%c3 src1_sel:DWORD"
            : "=v"(r) : "v"(w), "s"(0xF0u), "i"(K));
    }
    return r;
}

// The single-key kernel's Horner multiply on 5-bit windows.
// 26 windows cover x^0..x^127 (128 = 25·5 + 3): window P holds the coefficients x^(5P)..x^(5P+4),
// its value v has MSB = x^(5P); window 25 has three coefficients, in the top bits of its value.
constexpr int kWin5 = 26;
// x · F where f5 (LDS) holds F5[P][v] = (v·x^5P)·H^4 (reduced) as two tables of 8-byte halves: words
// 0-1 of position P at byte 2P*256 + 8v, words 2-3 at (2P+1)*256 + 8v. A table is one 256-byte row
// of the LDS, so the 32 lanes of a ds_read_b64 pass read it conflict-free whatever their entries
// (distinct entries are distinct bank pairs, equal entries one address), and no lane rotation is
// needed. 52 ds_read_b64 at 2 array cycles against the nibble table's 32 ds_read_b128 at 4.
// One address (v << 3) per window serves both halves; windows 6, 12 and 19 straddle two words.
__device__ __forceinline__ uint4 gf_mul_full5(uint4 x, uint4 acc, const uint2* f5) {
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    uint2 lo[kWin5], hi[kWin5];
    auto issue = [&](int P) {
        const int q = (5 * P) >> 5, r = (5 * P) & 31;  // the window's MSB = bit 31-r of word q
        uint32_t w;
        if (r > 27 && q < 3) w = __builtin_amdgcn_alignbit(xw[q], xw[q + 1], 56 - r);  // field -> bits 3-7
        else w = r <= 24 ? xw[q] >> (24 - r) : xw[q] << (r - 24);
        const uint32_t a = w & 0xF8u;
        lo[P] = lds_b64(f5, (uint32_t)(2 * P) * 256u + a);
        hi[P] = lds_b64(f5, (uint32_t)(2 * P + 1) * 256u + a);
    };
    // The volatile reads keep their program order, so the schedule is written out: the 8 reads of
    // 4 windows, then their fold; the other waves cover the latency, as with the nibble table (2 reads,
    // then their fold). C2 A/B over 5 rounds: steps of 2, 4 and 6 windows gave 840.7, 847.8 and
    // 846.6 GiB/s against the nibble table's 814.8 (profiles/ghash5/ab_c2.jsonl); issuing the next
    // step's reads before the fold gained nothing, and from 4 windows ahead on it spills.
    constexpr int kStep = 4;
#pragma unroll
    for (int g = 0; g < kWin5; g += kStep) {
#pragma unroll
        for (int P = g; P < g + kStep && P < kWin5; P++) issue(P);
#pragma unroll
        for (int P = g; P < g + kStep && P < kWin5; P += 2)  // kWin5 is even: windows fold in pairs
            acc = make_uint4(x3(acc.x, lo[P].x, lo[P + 1].x), x3(acc.y, lo[P].y, lo[P + 1].y),
                             x3(acc.z, hi[P].x, hi[P + 1].x), x3(acc.w, hi[P].y, hi[P + 1].y));
    }
    return acc;
}

// x · P where the LDS holds the 8 position tables T_r[v] = v·x^(4r)·P (reduced) at byte
// r*256 + v*16 from base + off (off per lane, a multiple of 256): nibble r of word q contributes T_r[v]·x^(32q), a shift by whole words, so the 32
// lookups XOR straight into a 224-bit product that is reduced once. No shifts (the Shoup form
// shifts every lookup by 4r bits): ~125 VALU per multiply instead of ~240, at 2 KiB per power.
// For P = H^4 the tables are the first 8 positions of the single-key full table.
__device__ __forceinline__ uint4 gf_mul_pos_off(uint4 x, const void* base, uint32_t off) {
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t hi = xw[q], lo = xw[q] << 4;
        const uint32_t ah[4] = {byte_hi_nibble<0>(hi), byte_hi_nibble<1>(hi), byte_hi_nibble<2>(hi),
                                byte_hi_nibble<3>(hi)};
        const uint32_t al[4] = {byte_hi_nibble<0>(lo), byte_hi_nibble<1>(lo), byte_hi_nibble<2>(lo),
                                byte_hi_nibble<3>(lo)};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 e1 = lds_at<uint4>(base, (uint32_t)(6 - 2 * k) * 256u + (ah[k] | off));
            const uint4 e2 = lds_at<uint4>(base, (uint32_t)(7 - 2 * k) * 256u + (al[k] | off));
            z[q] = x3(z[q], e1.x, e2.x);
            z[q + 1] = x3(z[q + 1], e1.y, e2.y);
            z[q + 2] = x3(z[q + 2], e1.z, e2.z);
            z[q + 3] = x3(z[q + 3], e1.w, e2.w);
        }
    }
    return gf_reduce(z);
}
__device__ __forceinline__ uint4 gf_mul_pos(uint4 x, const uint4* ptab) { return gf_mul_pos_off(x, ptab, 0u); }

// x · H^k where `tab` is the LDS byte offset (multiple of 256, < 2^24, relative to `base`) of a
// Shoup table M[v] = v·H^k. 32 independent lookups grouped by shift residue, reduced once.
__device__ __forceinline__ uint4 gf_mul_shoup(uint4 x, uint32_t tab, const uint4* base) {
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        hi[q] = xw[q] & 0xF0F0F0F0u;
        lo[q] = (xw[q] << 4) & 0xF0F0F0F0u;
    }
    uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 8; r++) {
        // nibble r of every word: byte (3 - r/2) of hi (even r) or lo (odd r)
        const int k = 3 - (r >> 1);
        uint4 m[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t src = (r & 1) ? lo[q] : hi[q];
            // address = tab | (nibble << 4): byte k of src into byte 0, tab's bytes 1..3 kept
            m[q] = lds_at<uint4>(base, perm(src, tab, 0x03020100u | (uint32_t)(4 + k)));
        }
        uint32_t a[7];
        a[0] = m[0].x;
        a[1] = m[0].y ^ m[1].x;
        a[2] = x3(m[0].z, m[1].y, m[2].x);
        a[3] = x3(m[0].w, m[1].z, m[2].y) ^ m[3].x;
        a[4] = x3(m[1].w, m[2].z, m[3].y);
        a[5] = m[2].w ^ m[3].z;
        a[6] = m[3].w;
        if (r == 0) {
#pragma unroll
            for (int i = 0; i < 7; i++) z[i] ^= a[i];
        } else {
            const uint32_t sh = 4 * r;
            z[0] ^= a[0] >> sh;
#pragma unroll
            for (int i = 1; i < 7; i++) z[i] ^= shr64(a[i - 1], a[i], sh);
            z[7] ^= a[6] << (32 - sh);
        }
        __builtin_amdgcn_sched_barrier(0);  // at most one residue's lookups in flight
    }
    return gf_reduce(z);
}

// Entry e (0..15) of the 4-bit Shoup table of P: XOR of P·x^j for the set bits (bit 3 ↔ x^0).
__device__ __forceinline__ uint4 gf_tab_entry(uint4 p, uint32_t e) {
    uint4 p1 = gf_mulx(p), p2 = gf_mulx(p1), p3 = gf_mulx(p2);
    uint32_t m8 = (e & 8) ? ~0u : 0u, m4 = (e & 4) ? ~0u : 0u, m2 = (e & 2) ? ~0u : 0u, m1 = (e & 1) ? ~0u : 0u;
    uint4 r;
    r.x = (p.x & m8) ^ (p1.x & m4) ^ (p2.x & m2) ^ (p3.x & m1);
    r.y = (p.y & m8) ^ (p1.y & m4) ^ (p2.y & m2) ^ (p3.y & m1);
    r.z = (p.z & m8) ^ (p1.z & m4) ^ (p2.z & m2) ^ (p3.z & m1);
    r.w = (p.w & m8) ^ (p1.w & m4) ^ (p2.w & m2) ^ (p3.w & m1);
    return r;
}

__device__ __forceinline__ uint4 ld_rec4(const uint32_t* rec, uint32_t i) {
    return *reinterpret_cast<const uint4*>(rec + i);
}

}  // namespace neb
