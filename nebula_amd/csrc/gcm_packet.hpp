// gcm_packet.hpp — one packet group of a wave sealed or opened (gcm_packet_group): the lane roles,
// block load / XOR / store, the GHASH table policies (Gh*), the TX checksum fix-up and the tag finish.
// Every GCM kernel of aes_gcm.hip runs its packets through it.
#pragma once
#include <type_traits>

#include "../../include/nebula_aead.h"
#include "aes_core.hpp"
#include "gcm_trace.hpp"
#include "gf128.hpp"
#include "layout.hpp"

namespace neb {

// ------------------------------------------------------------------------------------------
// Per-packet work shared by every kernel

struct GcmArgs {
    const neb_desc* desc;
    uint32_t npkt;
    uint8_t* arena;
    const uint32_t* keys;  // key table, kKeyRecDwords per key
    uint32_t max_keys;
    uint32_t key_hint;     // SINGLE: the one key_id
    int32_t* status;
    const uint32_t* npkt_dev;  // optional: the batch's packet count in device memory (min with npkt)
    // TX batches only (tx.hip): a descriptor's first `flags` plaintext bytes are read from its
    // destination (the patched header image), the rest from src (the TUN read itself)
    uint32_t hdr_from_dst;
    // single-key kernel: the waves of its grid (packets past its full passes are left to
    // gcm_single_tail_kernel), 0 = it takes every packet itself
    uint32_t tail_slots;
    // the device receive's admission mask (window.cpp): only packets with adm[p] != 0 are opened, the
    // others keep the status the receive's plan gave them (RX instantiations only)
    const uint8_t* adm;
};

struct PktShape {
    uint32_t na, m, n, R, pad;
};

// One round of one packet lane: keystream, payload XOR, GHASH input block. Returns X (BE words).
// Block roles of lane l in round r: 1-based GHASH index g and, for a ciphertext block, its counter.
struct LaneBlock {
    int32_t g;
    bool is_aad, is_ct, is_len;
    uint32_t k, ctr;
};
__device__ __forceinline__ LaneBlock lane_block(const PktShape& sh, uint32_t r, uint32_t l, uint32_t lg) {
    LaneBlock b;
    b.g = (int32_t)((r << lg) + l + 1u) - (int32_t)sh.pad;
    b.is_aad = b.g >= 1 && b.g <= (int32_t)sh.na;
    b.is_ct = b.g > (int32_t)sh.na && b.g <= (int32_t)(sh.na + sh.m);
    b.is_len = b.g == (int32_t)sh.n;
    b.k = (uint32_t)(b.g - (int32_t)sh.na);  // ciphertext block index (1-based)
    b.ctr = b.is_ct ? b.k + 1u : 1u;          // the length lane computes E_K(J0)
    return b;
}

// Input block of lane block b: the AAD block or the payload block (zero-padded), else zero.
// hdr: plaintext bytes [0, hdr) come from the destination (GcmArgs::hdr_from_dst).
__device__ __forceinline__ uint4 gcm_lane_load(const neb_desc& d, const LaneBlock& b, const uint8_t* arena,
                                               uint32_t hdr) {
    uint4 in = make_uint4(0, 0, 0, 0);
    if (b.is_aad) {
        const uint32_t off = 16u * (uint32_t)(b.g - 1);
        in = load_block(arena + d.aad_off + off, min(16u, d.aad_len - off));
    }
    if (b.is_ct) {
        const uint32_t off = 16u * (b.k - 1u);
        const uint32_t nb = min(16u, d.len - off);
        in = off < hdr ? load_block_hdr(arena + d.dst_off + off, arena + d.src_off + off, nb, hdr - off)
                       : load_block(arena + d.src_off + off, nb);
    }
    return in;
}

// Where the length lane keeps E_K(J0) from its round to the tag finish.
struct Ej0Reg {
    uint4 v = make_uint4(0, 0, 0, 0);
    __device__ __forceinline__ void set(uint4 k) { v = k; }
    __device__ __forceinline__ uint4 get() const { return v; }
};

// Payload XOR and GHASH input of one block given its input and keystream. Returns X (BE words).
template <bool OPEN>
__device__ __forceinline__ uint4 gcm_lane_io(const neb_desc& d, const LaneBlock& b, uint4 in, uint4 ks,
                                             uint8_t* arena, Ej0Reg& ej0) {
    uint4 X = make_uint4(0, 0, 0, 0);
    if (b.is_aad) X = bswap4(in);
    if (b.is_ct) {
        const uint32_t off = 16u * (b.k - 1u);
        const uint32_t nb = min(16u, d.len - off);
        const uint4 out = xor4(in, mask_block(ks, nb));
        store_block(arena + d.dst_off + off, out, nb);
        X = bswap4(OPEN ? in : out);
    }
    if (b.is_len) {
        const uint64_t abits = (uint64_t)d.aad_len * 8u, cbits = (uint64_t)d.len * 8u;
        X = make_uint4((uint32_t)(abits >> 32), (uint32_t)abits, (uint32_t)(cbits >> 32), (uint32_t)cbits);
        ej0.set(ks);
    }
    return X;
}

// Keystream block of lane block b. CM: counter-mode caching level — 0 none, 1 every counter of
// the wave below 2^16, 2 below 2^8.
template <int CM, class TL, class RK>
__device__ __forceinline__ uint4 gcm_lane_ks(const LaneBlock& b, uint32_t c1, uint32_t c2, const CtrConst& cc,
                                             const TL& T, const RK& rk) {
    if constexpr (CM == 2) return aes256_ctr8_block(cc, b.ctr, T, rk);
    else if constexpr (CM == 1) return aes256_ctr_block(cc, b.ctr, T, rk);
    else return aes256_block(0u, c1, c2, bswap32(b.ctr), T, rk);
}

// Tag finish on the packet's last lane, which holds E_K(J0) (seal: store; open: compare, zero
// the payload on mismatch).
template <bool OPEN>
__device__ __forceinline__ uint32_t gcm_finish(const neb_desc& d, uint4 S, uint4 ej0, uint32_t lane, uint32_t l,
                                               uint32_t LPP, uint8_t* arena) {
    const uint4 tag = xor4(ej0, bswap4(S));  // valid on lane LPP-1
    uint32_t fail = 0;
    if (l == LPP - 1u) {
        if constexpr (!OPEN) {
            store_block(arena + d.dst_off + d.len, tag, 16);
        } else {
            const uint4 rt = load_block(arena + d.src_off + d.len, 16);
            const uint4 df = xor4(rt, tag);
            fail = (df.x | df.y | df.z | df.w) != 0u;
        }
    }
    if constexpr (OPEN) {
        fail = (uint32_t)__shfl((int)fail, (int)(lane | (LPP - 1u)));
        if (fail) {
            for (uint32_t off = 16u * l; off < d.len; off += 16u * LPP)
                store_block(arena + d.dst_off + off, make_uint4(0, 0, 0, 0), min(16u, d.len - off));
        }
    }
    return fail;
}

// ------------------------------------------------------------------------------------------
// Packet groups: LPP = 2^lg lanes per packet (4 in the single-key kernel; 4, 8 or 16 per chunk in
// the mixed-key kernel), 64 / LPP packets per wave.
//
// Lane l of a packet owns padded GHASH blocks g' = LPP·r + l + 1 (n' = LPP·ceil(n/LPP); a
// 1300-byte packet has n = 84, so at LPP 4 nothing is padded). Horner stride H^LPP. The final
// Σ_l A_l·H^(LPP-l) multiplies with one table shared by every lane of a ds_read_b128 group at a
// time: no bank conflicts (per-lane power tables conflicted on every lookup and cost 17%).
// The round keys are wave-uniform (scalar registers) in every kernel: one key per batch or per
// request, or one key per chunk of a regrouped mixed-key batch (sched.hpp).

// GHASH tables a packet group multiplies with: horner(A) = A·H^LPP, and final(A) = the packet's
// Σ_l A_l·H^(LPP-l), valid at least on the packet's last lane (the one holding E_K(J0)).
//
// The final as one multiply per lane (LPP 4): lane l of a quad needs A_l·H^(4-l), and the quad
// XOR of those is the packet's Σ_l A_l·H^(4-l). A ds_read_b128 is served in four groups of 16 lanes
// (MI355X_MICROARCH.md, LDS); lanes of one group reading different tables at the same nibble would
// conflict, so the accumulators are first permuted (ds_bpermute) so that group g holds role g of
// all 16 packets and multiplies by H^(4-g) alone — conflict-free, as the Horner step — then pulled
// back and XORed over the quad. 8 bpermutes + 1 multiply instead of a quad Horner's 4 multiplies.
struct FinalPermLanes {
    uint32_t src1, src2, off;  // pull source (role g of packet idx), pull-back source, table offset
};
// tab_off[g]: byte offset from the LDS base of the tables of H^(4-g)
__device__ __forceinline__ FinalPermLanes final_perm_lanes(uint32_t lane, const uint32_t tab_off[4]) {
    // b128 lane groups: lanes 32h + 4·c + j with c = quad index mod 8, group 2h + parity(c), index
    // 4·(c >> 1) + j within it (groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the upper half)
    const uint32_t c = (lane >> 2) & 7u, h = lane >> 5;
    const uint32_t g = ((uint32_t)__popc(c) & 1u) + 2u * h;
    const uint32_t i = 4u * (c >> 1) + (lane & 3u);
    const uint32_t l = lane & 3u, q = lane >> 2, m = q >> 2;
    const uint32_t b = (l & 1u) ^ ((uint32_t)__popc(m) & 1u);
    FinalPermLanes f;
    f.src1 = 4u * i + g;
    f.src2 = 32u * (l >> 1) + 4u * (2u * m + b) + (q & 3u);
    f.off = g == 0u ? tab_off[0] : g == 1u ? tab_off[1] : g == 2u ? tab_off[2] : tab_off[3];
    return f;
}
template <int CTRL>
__device__ __forceinline__ uint4 dpp4(uint4 v) {
    return make_uint4((uint32_t)__builtin_amdgcn_mov_dpp((int)v.x, CTRL, 0xF, 0xF, false),
                      (uint32_t)__builtin_amdgcn_mov_dpp((int)v.y, CTRL, 0xF, 0xF, false),
                      (uint32_t)__builtin_amdgcn_mov_dpp((int)v.z, CTRL, 0xF, 0xF, false),
                      (uint32_t)__builtin_amdgcn_mov_dpp((int)v.w, CTRL, 0xF, 0xF, false));
}
// pull role g of every packet into b128 group g, multiply, pull back, XOR over the quad
template <class MUL>
__device__ __forceinline__ uint4 final_perm(uint4 A, const FinalPermLanes& fp, MUL&& mul) {
    const uint4 a = shfl4(A, fp.src1);
    uint4 v = shfl4(mul(a, fp.off), fp.src2);
    v = xor4(v, dpp4<0xB1>(v));     // quad_perm [1,0,3,2]
    return xor4(v, dpp4<0x4E>(v));  // quad_perm [2,3,0,1]
}

// One key per batch, LPP 4 (gcm_single_kernel): reduction-free full table of H^4 for the Horner
// step, position tables of H, H^2, H^3, H^4 for the permuted final.
struct GhFullPerm {
    const uint2* full;  // F5, the 5-bit window table of H^4 (gf_mul_full5)
    const void* base;  // the LDS base of FinalPermLanes::off
    FinalPermLanes fp;
    __device__ __forceinline__ uint4 horner(uint4 a, uint32_t) const {
        return gf_mul_full5(a, make_uint4(0, 0, 0, 0), full);
    }
    __device__ __forceinline__ uint4 final(uint4 A, uint32_t, uint32_t) const {
        return final_perm(A, fp, [&](uint4 a, uint32_t off) { return gf_mul_pos_off(a, base, off); });
    }
};

// 64 lanes per packet (the tail and per-packet kernels): lane l = 16a + b needs A_l·H^(64-l) =
// A_l·H^(16-b)·H^(16(3-a)). Each lane multiplies by its own M_(16-b) (the record's Shoup tables of
// H^1..H^16), the 16 lanes of a quarter XOR their products (S_a), quarter a < 3 multiplies its sum by
// H^(16(3-a)), and the quarters XOR: 2 dependent multiplies instead of a pairwise tree's 7.
struct Gh64Tabs {        // the table set in LDS, one per key
    uint4 pos[8 * 16];   // 2 KiB: position tables of H^64 (the Horner stride)
    uint4 m16[16 * 16];  // 4 KiB: M_1..M_16, 256 B each
    uint4 hi[3 * 16];    // M_16, M_32, M_48: the quarters' powers
};
// Thread i of n (n >= 48) copies its share of the set from the key record.
__device__ __forceinline__ void stage_gh64(Gh64Tabs& t, const uint32_t* rec, uint32_t i, uint32_t n) {
    for (uint32_t k = i; k < 128u; k += n) t.pos[k] = ld_rec4(rec, kRecPos64 + 4u * k);
    for (uint32_t k = i; k < 256u; k += n) t.m16[k] = ld_rec4(rec, kRecShoup + 4u * k);
    if (i < 48u)
        t.hi[i] = ld_rec4(rec, (i < 16u ? kRecShoup + 15u * 64u : i < 32u ? kRecShoup32 : kRecShoup48) + 4u * (i & 15u));
}
struct GhShoup64 {
    const Gh64Tabs* t;
    __device__ __forceinline__ uint4 horner(uint4 a, uint32_t) const { return gf_mul_pos(a, t->pos); }
    __device__ __forceinline__ uint4 final(uint4 A, uint32_t lane, uint32_t lg) const {
        const uint32_t b = lane & 15u, a = (lane >> 4) & 3u;
        uint4 V = gf_mul_shoup(A, (15u - b) * 256u, t->m16);
        V = xor4(V, shfl_xor4(V, 8));
        V = xor4(V, shfl_xor4(V, 4));
        V = xor4(V, shfl_xor4(V, 2));
        V = xor4(V, shfl_xor4(V, 1));
        const uint4 W = gf_mul_shoup(V, (a < 3u ? 2u - a : 0u) * 256u, t->hi);  // S_a·H^(16(3-a))
        V = a < 3u ? W : V;
        V = xor4(V, shfl_xor4(V, 16));
        return xor4(V, shfl_xor4(V, 32));
    }
};

// Mixed-key chunks (gcm_chunk_kernel), tables in the wave's LDS slice, restaged per chunk.
// Full chunks (16 packets at 4 lanes, the single-key kernel's layout): Horner on the position
// tables of H^4, the permuted final on the Shoup tables M_1..M_4 (b128 group g multiplies role g of
// every packet by M_(4-g)).
struct GhChunk4 {
    const uint4* shoup;  // M_1, M_2, M_3, M_4 (record Shoup tables 0-3)
    const uint4* pos;    // position tables of H^4
    __device__ __forceinline__ uint4 horner(uint4 a, uint32_t) const { return gf_mul_pos(a, pos); }
    __device__ __forceinline__ uint4 final(uint4 A, uint32_t lane, uint32_t) const {
        // the lane permutation is recomputed here rather than held across the chunk loop, where
        // its registers would be spilled (the compiler would hoist it: the opaque copy of `lane`
        // keeps it here)
        const uint32_t ln = lane;
        const uint32_t tab_off[4] = {3u * 256u, 2u * 256u, 256u, 0u};  // M_4, M_3, M_2, M_1
        return final_perm(A, final_perm_lanes(ln, tab_off),
                          [&](uint4 a, uint32_t off) { return gf_mul_shoup(a, off, shoup); });
    }
};
// Tail chunks (1-8 packets at 8 or 16 lanes): Horner on the position tables of H^(2^lg); the final
// as quads, then a short tree over the packet's quads (round 6). Lane l = 4a + b of a packet needs
// A_l·H^(LPP-l) = A_l·H^(4-b)·H^(4(LPP/4-1-a)): the permuted one-multiply final of the 4-lane chunks
// gives every quad Q_a = Σ_b A_(4a+b)·H^(4-b) (final_perm treats each quad as a packet), then
// LPP 8: Q_0·H^4 ⊕ Q_1; LPP 16: (Q_0·H^4 ⊕ Q_1)·H^8 ⊕ (Q_2·H^4 ⊕ Q_3). Every lane of a level multiplies
// by the same table (M_4, then M_8), so the lookups stay conflict-free: 2 or 3 dependent multiplies
// instead of the pairwise tree's 4 or 5 (that tree cost ≈ 2 rounds of VALU per tail chunk, and tail
// chunks are half of a C5 shard's chunks).
struct GhChunkTail {
    const uint4* shoup;  // M_1, M_2, M_3, M_4, M_8
    const uint4* pos;    // position tables of H^(2^lg)
    __device__ __forceinline__ uint4 horner(uint4 a, uint32_t) const { return gf_mul_pos(a, pos); }
    __device__ __forceinline__ uint4 final(uint4 A, uint32_t lane, uint32_t lg) const {
        const uint32_t ln = lane;
        const uint32_t tab_off[4] = {3u * 256u, 2u * 256u, 256u, 0u};  // M_4, M_3, M_2, M_1
        const uint4 Q = final_perm(A, final_perm_lanes(ln, tab_off),
                                   [&](uint4 a, uint32_t off) { return gf_mul_shoup(a, off, shoup); });
        const uint32_t a = (ln >> 2) & ((1u << (lg - 2u)) - 1u);  // the quad's index in its packet
        // (selects per component: a select of two uint4 values went through a scratch array)
        const uint4 W = sel4((a & 1u) != 0u, Q, gf_mul_shoup(Q, 3u * 256u, shoup));  // even quads: Q·H^4
        const uint4 P = xor4(W, shfl_xor4(W, 4));  // quads (0,1): Q_0·H^4 ⊕ Q_1, (2,3): Q_2·H^4 ⊕ Q_3
        if (lg == 3u) return P;
        const uint4 U = sel4((a & 2u) != 0u, P, gf_mul_shoup(P, 4u * 256u, shoup));  // quads 0, 1: ·H^8
        return xor4(U, shfl_xor4(U, 8));
    }
};

// ---- the TX checksum in the seal (CS; tx.hip kTxCsumFlag) ----------------------------------
// The TX segment kernel leaves in the L4 checksum field the partial sum of everything but the
// payload bytes the seal reads from the TUN read ([hdr, len)); the seal adds those bytes' 16-bit
// words as it encrypts them. The field's block was encrypted with the partial (round 0): the
// packet's last lane then stores the field's final ciphertext bytes and moves the tag by the
// change, S' = S ^ Δ·H^e (GHASH is linear; e = n + 1 - the field block's index), with the Shoup
// tables of H^(2^j), j < 10, in LDS (e < 1024: tx.hip's seal_cs admits no other segment; under
// 16 KB alone is not enough, a field in block 0 or 1 of 1024 blocks has e = 1025 or 1024).
// desc.flags = hdr | field << 12 | kind << 24 | parity << 26, or hdr alone (kind 1: TCP or a plain packet, 2:
// UDP, whose computed zero goes out as 0xFFFF; parity: the checksum start's, for the word pairing).
constexpr uint32_t kCsHdrMask = 0xFFFu;
__device__ __forceinline__ uint32_t le16_sum(uint4 v) {
    return (v.x & 0xFFFFu) + (v.x >> 16) + (v.y & 0xFFFFu) + (v.y >> 16) + (v.z & 0xFFFFu) + (v.z >> 16) +
           (v.w & 0xFFFFu) + (v.w >> 16);
}
__device__ __forceinline__ uint32_t block_byte(uint4 v, uint32_t q) {
    const uint32_t w = q < 4u ? v.x : q < 8u ? v.y : q < 12u ? v.z : v.w;
    return (w >> (8u * (q & 3u))) & 0xFFu;
}
__device__ __forceinline__ uint32_t cs_fold16(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return s;
}
// The tag lane: the final checksum from the packet's payload sum `acc` (little-endian words) and
// the field word `fk` (partial << 16 | keystream bytes there); stores the field's ciphertext and
// returns Δ·H^e for the tag.
__device__ __forceinline__ uint4 gcm_csum_fix(const neb_desc& d, uint32_t n, uint32_t na, uint32_t acc, uint32_t fk,
                                              uint8_t* arena, const uint4* pow2) {
    const uint32_t kind = (d.flags >> 24) & 3u, f = (d.flags >> 12) & 0xFFFu;
    uint32_t sum = cs_fold16(acc);
    if (!((d.flags >> 26) & 1u)) sum = ((sum & 0xFFu) << 8) | (sum >> 8);  // big-endian words
    const uint32_t fval = fk >> 16, ks16 = fk & 0xFFFFu;
    uint32_t c = ~cs_fold16(sum + fval) & 0xFFFFu;
    if (kind == 2u && c == 0u) c = 0xFFFFu;
    const uint32_t delta = fval ^ c;
    __threadfence_block();  // the field's block was stored by a lane of this wave in an earlier round
    uint8_t* ct = arena + d.dst_off + f;
    ct[0] = (uint8_t)((ks16 ^ c) >> 8);
    ct[1] = (uint8_t)(ks16 ^ c);
    // Δ as a GHASH block (big-endian words): bytes q and q + 1 (q < 15: the segment kernel keeps
    // the field inside one block)
    const uint32_t q = f & 15u, q1 = q + 1u;
    const uint32_t hi = (delta >> 8) << (24u - 8u * (q & 3u)), lo = (delta & 0xFFu) << (24u - 8u * (q1 & 3u));
    uint4 corr = make_uint4(((q >> 2) == 0u ? hi : 0u) | ((q1 >> 2) == 0u ? lo : 0u),
                            ((q >> 2) == 1u ? hi : 0u) | ((q1 >> 2) == 1u ? lo : 0u),
                            ((q >> 2) == 2u ? hi : 0u) | ((q1 >> 2) == 2u ? lo : 0u),
                            ((q >> 2) == 3u ? hi : 0u) | ((q1 >> 2) == 3u ? lo : 0u));
    const uint32_t e = n - na - (f >> 4);  // n + 1 - (na + f / 16 + 1)
    for (uint32_t j = 0; j < 10u; j++)
        if ((e >> j) & 1u) corr = gf_mul_shoup(corr, j * 256u, pow2);
    return corr;
}

// Seal or open packet `p` (lanes (lane >> lg) << lg ... + LPP-1 of the wave). `expect_key`: the key
// this wave's round keys and tables belong to; key_ok: that key is installed with the right
// algorithm. lg is wave-uniform.
// own (optional): the packet's descriptor itself, not args.desc[p] (the per-packet kernel's, rebased).
// RX: the device receive's open (args.adm), an instantiation of its own so the plain opens keep their
// registers.
template <bool OPEN, bool CS = false, bool RX = false, class GH, class TL, class RK>
__device__ __forceinline__ void gcm_packet_group(const GcmArgs& args, uint32_t p, bool valid, uint32_t expect_key,
                                                 bool key_ok, const RK& rk, const GH& gh, const TL& T,
                                                 uint32_t lane, uint32_t lg, const uint4* cs_pow = nullptr,
                                                 const neb_desc* own = nullptr) {
    const uint32_t LPP = 1u << lg;
    const uint32_t l = lane & (LPP - 1u);
    NEB_MARK(grp_begin);
    GroupTrace tr;
    tr.begin();
    neb_desc d = {};
    uint32_t admit = 1u;
    if (valid) {
        d = own ? *own : args.desc[p];
        if constexpr (RX) admit = args.adm[p];  // (beside the descriptor's load, not behind it)
    }
    tr.desc_in();
    // the device receive opens only what its windows admitted (the rest keep the plan's status)
    if constexpr (RX) valid = valid && admit != 0u;
    uint32_t st = NEB_STATUS_OK;
    if (!key_ok || d.key_id != expect_key) st = NEB_STATUS_BAD_KEY;
    if (!OPEN && st == NEB_STATUS_OK && d.counter >= kRejectAfterMessages) st = NEB_STATUS_EXHAUSTED;
    const bool run = valid && st == NEB_STATUS_OK;
    // (no checksum kind: the whole word is the prefix, a plain packet's can pass 12 bits)
    const uint32_t hdr = !args.hdr_from_dst ? 0u : ((d.flags >> 24) & 3u) ? d.flags & kCsHdrMask : d.flags;
    // CS: this lane's payload word sum, and (the field's lane) partial << 16 | keystream bytes
    uint32_t cs_acc = 0, cs_fk = 0;
    const bool cs_on = CS && !OPEN && ((d.flags >> 24) & 3u) != 0u;
    const uint32_t cs_f = (d.flags >> 12) & 0xFFFu;
    PktShape sh;
    sh.na = (d.aad_len + 15u) >> 4;
    sh.m = (d.len + 15u) >> 4;
    sh.n = sh.na + sh.m + 1u;
    sh.R = run ? (sh.n + LPP - 1u) >> lg : 0u;
    sh.pad = (sh.R << lg) - sh.n;
    Ej0Reg ej0;
    // the uniform-round loop (below): the single-key kernel's plain seal and open only
    constexpr bool kUni = std::is_same_v<GH, GhFullPerm> && !CS && !RX;

    // nonce 00000000 || BE64(n) as little-endian words; counter block word 3 = BE32(ctr)
    const uint32_t c1 = bswap32((uint32_t)(d.counter >> 32));
    const uint32_t c2 = bswap32((uint32_t)d.counter);
    uint4 A = make_uint4(0, 0, 0, 0);
    auto rounds = [&](auto cm) {
        constexpr int CM = decltype(cm)::value;
        CtrConst cc{};
        if constexpr (CM == 2) cc = aes_ctr_prep8(c1, c2, T, rk);
        else if constexpr (CM == 1) cc = aes_ctr_prep(c1, c2, T, rk);
        NEB_MARK(ctr_done);
        // The common round: every active lane holds a full payload block with a 16-B aligned
        // destination (the arena base counts too: a caller may pass an arena at any byte address);
        // a source off 16-B alignment (a TX segment inside its TUN read) is read as two aligned
        // blocks and shifted. Its block is loaded at the top of the round (fast_load), so the load's
        // latency overlaps the round's GHASH and AES instead of following them: a wave's round is
        // a chain of dependent LDS lookups, and the mixed-key kernel's last chunks run with few
        // waves per CU to hide it (C3 +2.7%, C2 equal; tools/wave_trace.py).
        auto fast_round = [&](const LaneBlock& b) {
            const uint32_t off = 16u * (b.k - 1u);
            return __all(b.is_ct && off + 16u <= d.len && off >= hdr &&
                         ((d.dst_off | (uint32_t)(uintptr_t)args.arena) & 15u) == 0u);
        };
        auto fast_load = [&](const LaneBlock& b) {
            const uint8_t* sp = args.arena + d.src_off + 16u * (b.k - 1u);
            return __all(((uint32_t)(uintptr_t)sp & 3u) == 0u) ? load_u4_a4(sp) : load_shifted16(sp);
        };
        // round r's payload XOR and GHASH fold, given G = A·H^LPP (the rounds before), the keystream
        // and (a common round) the block loaded at the round's top
        auto io = [&](const LaneBlock& b, uint4 G, uint4 ks, bool fast, uint4 pre) {
            const uint32_t off = 16u * (b.k - 1u);
            if (fast) {
                const uint4 in = pre;
                if constexpr (CS) {
                    if (cs_on) cs_acc += le16_sum(in);
                }
                const uint4 out = xor4(in, ks);
                *reinterpret_cast<uint4*>(args.arena + d.dst_off + off) = out;
                A = xor4(G, bswap4(OPEN ? in : out));
                return;
            }
            const uint4 in = gcm_lane_load(d, b, args.arena, hdr);
            if constexpr (CS) {
                if (cs_on && b.is_ct) {
                    const uint32_t off = 16u * (b.k - 1u);
                    const uint32_t hi = min(16u, d.len - off), lo = hdr > off ? min(hdr - off, 16u) : 0u;
                    if (lo < hi) {  // the bytes of [hdr, len) in this block
                        const uint4 v = mask_block(in, hi);
                        cs_acc += le16_sum(xor4(v, mask_block(v, lo)));
                    }
                    if (cs_f - off < 16u) {
                        const uint32_t q = cs_f - off;
                        cs_fk = (block_byte(in, q) << 24) | (block_byte(in, q + 1u) << 16) | (block_byte(ks, q) << 8) |
                                block_byte(ks, q + 1u);
                    }
                }
            }
            A = xor4(G, gcm_lane_io<OPEN>(d, b, in, ks, args.arena, ej0));
        };
        auto horner = [&](uint32_t r) -> uint4 { return r == 0 ? make_uint4(0, 0, 0, 0) : gh.horner(A, lg); };
        // one round on the LDS: GHASH of the previous rounds first, then this round's T-table AES
        // (one phase's registers at a time)
        auto tround = [&](uint32_t r) {
            NEB_MARK(round_begin);
            if (r < sh.R) {
                const LaneBlock b = lane_block(sh, r, l, lg);
                const bool fast = fast_round(b);
                uint4 pre = make_uint4(0, 0, 0, 0);
                if (fast) pre = fast_load(b);
                const uint4 G = horner(r);
                __builtin_amdgcn_sched_barrier(0);
                // a round with no ciphertext or length block in the wave needs no keystream: the
                // AAD-only rounds of GMAC (relay verify, connection_state.go:121-148) skip the AES
                uint4 ks = make_uint4(0, 0, 0, 0);
                if (__any(b.is_ct || b.is_len)) ks = gcm_lane_ks<CM>(b, c1, c2, cc, T, rk);
                io(b, G, ks, fast, pre);
            }
            NEB_MARK(round_end);
        };
        // Uniform waves (single-key kernel, counter tier 2, plain seal and open): when all 16 packets
        // run with one (aad_len, len), no header bytes from the destination, 16-B aligned destinations
        // and 4-B aligned sources, a round's block roles depend on (r, l) alone. The rounds [u0, u1)
        // in which every lane holds a full payload block then run with a scalar trip count, one
        // running source and destination pointer per lane and ctr += 4: no roles, votes, alignment
        // tests or address rebuilds. The rounds before (AAD, pad) and after (partial block, length
        // block, E_K(J0)) stay with tround. One test per wave; any other wave runs the general loop,
        // which is a loop of its own: entered from inside it, the uniform rounds changed its
        // register allocation and cost the 1-key relay (AAD-only rounds) 6%.
        if constexpr (kUni && CM == 2) {
            uint32_t u0 = ~0u, u1 = 0u;
            const uint32_t ulen = __builtin_amdgcn_readfirstlane(d.len);
            const uint32_t uaad = __builtin_amdgcn_readfirstlane(d.aad_len);
            const uintptr_t ab = reinterpret_cast<uintptr_t>(args.arena);
            if (__all(run && d.len == ulen && d.aad_len == uaad && hdr == 0u &&
                      (((uint32_t)d.dst_off | (uint32_t)ab) & 15u) == 0u &&
                      (((uint32_t)d.src_off + (uint32_t)ab) & 3u) == 0u)) {
                const uint32_t na = (uaad + 15u) >> 4, n = na + ((ulen + 15u) >> 4) + 1u;
                const uint32_t pad = (((n + LPP - 1u) >> lg) << lg) - n;
                const uint32_t a = (na + pad + LPP - 1u) >> lg, b = (na + pad + (ulen >> 4)) >> lg;
                if (a < b) u0 = a, u1 = b;
            }
            if (u0 != ~0u) {
                // tround over [0, u0), the uniform rounds [u0, u1), tround over [u1, R): written as
                // one loop that jumps from u0 to u1, so that tround is inlined once here and not twice
                const uint32_t uR = __builtin_amdgcn_readfirstlane(sh.R);
                for (uint32_t r = 0; r < uR; r++) {
                    if (r == u0) {
                        const uint32_t k0 = (u0 << lg) + l + 1u - sh.pad - sh.na;  // this lane's first block
                        const uint8_t* sp = args.arena + d.src_off + 16u * (k0 - 1u);
                        uint8_t* dp = args.arena + d.dst_off + 16u * (k0 - 1u);
                        uint32_t ctr = k0 + 1u;
                        for (uint32_t i = u0; i < u1; i++) {
                            NEB_MARK(uround_begin);
                            const uint4 in = load_u4_a4(sp);
                            const uint4 G = gh.horner(A, lg);
                            __builtin_amdgcn_sched_barrier(0);
                            const uint4 out = xor4(in, aes256_ctr8_block(cc, ctr, T, rk));
                            *reinterpret_cast<uint4*>(dp) = out;
                            A = xor4(G, bswap4(OPEN ? in : out));
                            sp += 16u * LPP;
                            dp += 16u * LPP;
                            ctr += LPP;
                            NEB_MARK(uround_end);
                        }
                        r = u1;
                    }
                    tround(r);
                }
                return;
            }
        }
        // rounds until no packet of the wave has one left (a ballot, no cross-lane reduction; a
        // shuffle max of the round counts first was 4-7% slower in the chunk kernel)
        for (uint32_t r = 0; __any(r < sh.R); r++) tround(r);
    };
    tr.rounds_begin();
    // counter caching needs every block counter of every packet in the wave below 2^8 / 2^16
    if (__all(sh.m + 1u < 256u)) rounds(std::integral_constant<int, 2>{});
    else if (__all(sh.m + 1u < 65536u)) rounds(std::integral_constant<int, 1>{});
    else rounds(std::integral_constant<int, 0>{});
    if constexpr (CS) {
        for (uint32_t sft = 1; sft < LPP; sft <<= 1) {
            cs_acc += (uint32_t)__shfl_xor((int)cs_acc, (int)sft);
            cs_fk |= (uint32_t)__shfl_xor((int)cs_fk, (int)sft);
        }
    }
    tr.rounds_done();
    NEB_MARK(rounds_done);
    uint4 V = gh.final(A, lane, lg);  // every lane: the tree shuffles across the packet's lanes
    NEB_MARK(final_done);
    tr.final_done(lane, sh.R);
    if constexpr (CS) {
        if (run && cs_on && l == LPP - 1u) V = xor4(V, gcm_csum_fix(d, sh.n, sh.na, cs_acc, cs_fk, args.arena, cs_pow));
    }
    if (run && gcm_finish<OPEN>(d, V, ej0.get(), lane, l, LPP, args.arena)) st = NEB_STATUS_AUTH_FAILED;
    if (valid && l == LPP - 1u) args.status[p] = (int32_t)st;
    NEB_MARK(grp_end);
    tr.finished();
}

__device__ __forceinline__ void load_round_keys(const uint32_t* rec, uint32_t rks[60]) {
#pragma unroll
    for (int i = 0; i < 60; i++) rks[i] = __builtin_amdgcn_readfirstlane(rec[kRecRoundKeys + i]);
}

}  // namespace neb
