// aes_gcm.hip — AES-256-GCM seal/open of a packet batch on gfx950 (MI355X).
//
// Replaces the arithmetic behind noiseutil/aesgcm.go:24-49 (EncryptDanger/DecryptDanger = Go
// crypto/cipher GCM Seal/Open with nonce 00000000 || BE64(n)) for a whole batch of packets.
//
// Work decomposition:
//  * A "packet group" is 64 / LPP packets of one wave, LPP = 2^lg lanes each (4 in the single-key
//    kernel and in full mixed-key chunks; 8 or 16 for short tail chunks; 64 in the tail kernel).
//  * A packet's GHASH input is n = a + m + 1 blocks (a AAD blocks, m ciphertext blocks, 1 length
//    block), front-padded with zero blocks to n' = LPP·R. In round r lane l owns padded block
//    g' = LPP·r + l + 1: it runs the AES-CTR keystream for that block (if it is a ciphertext block),
//    loads / XORs / stores the 16 payload bytes, and folds the block into its Horner accumulator
//    A_l = A_l·H^LPP ⊕ X. The length block always lands on the packet's last lane; that lane also
//    computes E_K(J0) for the tag.
//  * After R rounds GHASH = Σ_l A_l·H^(LPP-l): one multiply per lane after a lane permutation
//    (LPP 4), quads and a short tree (LPP 8, 16), or three dependent multiplies (LPP 64).
//  * AES: T-tables in LDS, 32 swizzled copies so every ds_read_b32 is bank-conflict-free and its
//    address is one v_perm_b32 (four tables, 128 KiB, in the single-key kernel; two tables, 64 KiB,
//    T1/T3 by one rotate, elsewhere). Round keys are wave-uniform (scalar registers).
//  * GHASH tables (precomputed at key install): a reduction-free "full" nibble table of H^4, and
//    position / Shoup tables of the other powers, staged in LDS per workgroup (one key) or per
//    wave and chunk (mixed keys).
//
// One translation unit in pieces: gcm_ops.hpp (instruction helpers), aes_core.hpp (the T-table AES),
// gf128.hpp (the GF(2^128) arithmetic), gcm_packet.hpp (gcm_packet_group and the GHASH policies) and
// gcm_trace.hpp (the instrumented builds). This file: the kernels, the key install, the launchers.
#include <hip/hip_runtime.h>

#include <atomic>
#include <hip/hip_ext.h>

#include <cstring>
#include <stdint.h>

#include <type_traits>

#include "../../include/nebula_aead.h"
#include "aes_core.hpp"
#include "cipher.hpp"
#include "device_common.hpp"
#include "gcm_packet.hpp"
#include "gcm_trace.hpp"
#include "gf128.hpp"
#include "knobs.hpp"
#include "layout.hpp"
#include "rxwin.hpp"
#include "sched.hpp"
#include "timing.hpp"

namespace neb {

// ---- one tunnel key for the whole batch -------------------------------------------------------

// Four-table AES (TLook4, 128 KiB) + the GHASH tables: one 1024-lane workgroup per CU, 4 waves per
// SIMD, at most 128 VGPRs.
constexpr uint32_t kLg = 2;             // log2 lanes per packet
constexpr uint32_t kLpp = 1u << kLg;    // = kFullPow, the full table's power
constexpr uint32_t kPpw = 64u / kLpp;   // packets per wave
static_assert(kLpp == kFullPow, "the single-key Horner stride is the full table's power");
constexpr int kSingleWaves = 16;
constexpr int kSingleWpe = 4;  // launch bound: waves per SIMD
constexpr int kSingleThreads = kSingleWaves * kWave;

struct SingleLds {
    uint2 full[2 * kWin5 * 32];  // 13 KiB  F5[P][v] for H^4, halves (first: its offsets fit the ds_read offset field)
    uint4 pos1[8 * 16];        // 2 KiB   position tables of H
    uint2 ttab[2 * 256 * 32];  // 128 KiB (T0,T1) and (T2,T3) pairs, 32 copies each
    uint4 pos23[2][8 * 16];    // 4 KiB   position tables of H^2 and H^3 (the permuted final)
    uint4 pos4[8 * 16];        // 2 KiB   position tables of H^4 (the final's; positions 0-7 of the nibble table)
};
struct SingleLdsCs : SingleLds {
    uint4 pow2[10 * 16];  // 2.5 KiB  Shoup tables of H^(2^j), j < 10 (the TX checksum correction)
};

// CS: the TX seal with the L4 checksums (gcm_csum_fix); RX: the device receive's open (GcmArgs::adm)
template <bool OPEN, bool CS = false, bool RX = false>
__global__ __launch_bounds__(kSingleThreads, kSingleWpe) void gcm_single_kernel(GcmArgs args) {
    __shared__ std::conditional_t<CS, SingleLdsCs, SingleLds> lds;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    const uint32_t* srec = args.keys + (size_t)args.key_hint * kKeyRecDwords;
    WaveTimeline wt;
    wt.kernel_begin(wave);
    // the record's GHASH tables: loaded before the T-table fill and stored after it, so their
    // latency overlaps the fill's instead of following it
    uint4 r_full = make_uint4(0, 0, 0, 0), r_h = make_uint4(0, 0, 0, 0), r_p = make_uint4(0, 0, 0, 0);
    // F5[P][v] from the record's nibble table: x^b·H^4 is its entry F_(b/4)[8 >> (b%4)], and thread
    // t < 26·32 XORs those of the (at most five) coefficients x^(5P+j) that v = t mod 32 selects
    static_assert(kSingleThreads >= kWin5 * 32, "one window-table entry per thread");
    const uint32_t f5_p = tid >> 5, f5_v = tid & 31u;
    if (tid < (uint32_t)kWin5 * 32u) {
#pragma unroll
        for (uint32_t j = 0; j < 5u; j++) {
            const uint32_t b = 5u * f5_p + j, bc = min(b, 127u);
            const uint4 c = ld_rec4(srec, kRecFull + 4u * ((bc >> 2) * 16u + (8u >> (bc & 3u))));
            const uint32_t m = (b < 128u && ((f5_v >> (4u - j)) & 1u)) ? ~0u : 0u;
            r_full = make_uint4(r_full.x ^ (c.x & m), r_full.y ^ (c.y & m), r_full.z ^ (c.z & m), r_full.w ^ (c.w & m));
        }
    }
    if (tid < 128u) r_h = ld_rec4(srec, kRecPos1 + 4u * tid);
    if (tid < 384u) r_p = ld_rec4(srec, (tid < 128u ? kRecPos2 : tid < 256u ? kRecPos3 : kRecFull) + 4u * (tid & 127u));
    const TLook4 T{lds.ttab, ttab4_lane_base(lane)};
    fill_ttab<2u * 256u * 32u, kSingleThreads>(lds.ttab, tid, ttab4_entry);
    if (tid < (uint32_t)kWin5 * 32u) {
        lds.full[(2u * f5_p) * 32u + f5_v] = make_uint2(r_full.x, r_full.y);
        lds.full[(2u * f5_p + 1u) * 32u + f5_v] = make_uint2(r_full.z, r_full.w);
    }
    if (tid >= 256u && tid < 384u) lds.pos4[tid & 127u] = r_p;
    if (tid < 128u) lds.pos1[tid] = r_h;
    if (tid < 256u) lds.pos23[tid >> 7][tid & 127u] = r_p;

    const uint4* cs_pow = nullptr;
    if constexpr (CS) {
        if (tid < 160u) lds.pow2[tid] = ld_rec4(srec, rec_shoup_pow2(tid >> 4) + 4u * (tid & 15u));
        cs_pow = lds.pow2;
    }
    uint32_t rks[60];
    load_round_keys(srec, rks);
    __syncthreads();
    const RkRegs rk{rks};
    const uint32_t tab_off[4] = {(uint32_t)offsetof(SingleLds, pos4), (uint32_t)offsetof(SingleLds, pos23[1]),
                                 (uint32_t)offsetof(SingleLds, pos23[0]), (uint32_t)offsetof(SingleLds, pos1)};
    const GhFullPerm gh{lds.full, &lds, final_perm_lanes(lane, tab_off)};

    // The slot must still hold an AES-GCM key when the batch runs (a key destroyed, or its slot
    // reused by another algorithm, while the batch was queued): every packet gets BAD_KEY then.
    const bool key_ok = __builtin_amdgcn_readfirstlane(srec[kRecAlg]) == NEB_ALG_AESGCM;
    uint32_t npkt = args.npkt;
    if (args.npkt_dev) npkt = min(npkt, __builtin_amdgcn_readfirstlane(*args.npkt_dev));
    const uint32_t ngroups = (npkt + kPpw - 1u) / kPpw;
    const uint32_t slots = gridDim.x * kSingleWaves;  // waves of the grid
    uint32_t main_groups = ngroups;
    if (args.tail_slots && ngroups > slots && ngroups % slots)
        main_groups = ngroups / slots * slots;  // full passes only: the tail kernel takes the rest
    // groups go to workgroups first (group g: workgroup g mod G, wave g / G), so a batch of fewer
    // groups than waves spreads over as many CUs as it can instead of filling a few (a 2048-packet
    // batch on 8 CUs ran as long as a whole 64 Ki pass)
    wt.tables_filled(lane);
    auto groups = [&](const auto& rkp) {
        for (uint32_t grp = blockIdx.x + wave * gridDim.x; grp < main_groups; grp += slots) {
            wt.chunk_begin();
            const uint32_t p = grp * kPpw + lane / kLpp;
            gcm_packet_group<OPEN, CS, RX>(args, p, p < npkt, args.key_hint, key_ok, rkp, gh, T, lane, kLg, cs_pow);
            wt.chunk_end(lane, kPpw << 8 | kLg << 4 | 1u, grp);  // (a group of 16 at 4 lanes, as a full chunk)
        }
    };
    // A workgroup's waves w, w+4, w+8, w+12 share a SIMD in that age order (wave >> 2 is the
    // rank), and the SIMD arbiter serves the older first at equal priority: ranks 0-3 finished
    // their groups in 74 / 78 / 84 / 88 µs (tools/wave_trace.py, C2 seal, settled clock). Ranks 2
    // and 3 keep priority 1 instead of 0 between their lookup phases, so they are not passed over
    // by the older pair there. Alternating A/B against the same code at 0 (tools/r5_prio_ab.sh,
    // profiles/r5/ab_balance): seal 96.5-98.7 -> 94.2-95.6 µs. Every other split tried — lookup levels by
    // rank, four distinct levels, 0/1/1/1, 0/0/2/2 — was equal or slower.
    if (__builtin_amdgcn_readfirstlane(wave) >> 3) groups(RkRegsPrio<NEB_PRIO, 1>{rk});
    else groups(rk);
}

// The tail pass: the packets after gcm_single_kernel's full passes over args.tail_slots waves (the
// groups that would otherwise run alone after everything else: 65 565 packets = 4098 groups of 16
// on 4096 waves), 2^kTailLg lanes per packet: the two-table AES (64 KiB), Horner stride
// H^(2^kTailLg) on its position tables, the 2-deep final on the Shoup tables of H .. H^16, H^32 and
// H^48 (GhShoup64). A tail is small and runs on few waves, so its time is one packet's latency: at 64
// lanes a 1300-B packet takes 2 rounds instead of 6 at 16 (bench.py --mode tx: 1457 vs 1456
// superpackets, 0.243 vs 0.207 ms before it).
constexpr uint32_t kTailLg = 6, kTailPpw = kWave >> kTailLg;
// GcmArgs::tail_slots value for a batch small enough to run entirely in the tail kernel: one packet
// per wave over 64 lanes is 2 rounds for 1300 B instead of 21, and a batch under a few thousand
// packets is bound by one wave's latency, not by throughput
constexpr uint32_t kTailAll = 0xFFFFFFFFu;
// packets (host-known count) up to which the tail kernel takes them all (A/B: 6144 55.8 vs 71.3 us
// per seal, 8192 equal, 12288 101 vs 75)
constexpr uint32_t kSmallBatch = 6144;
constexpr int kTailWaves = 8;
struct TailLds {
    uint2 ttab[256 * 32];  // 64 KiB T-table pairs, 32 copies
    Gh64Tabs gh;           // 6.75 KiB
};
static_assert(kTailLg == 6, "GhShoup64: 64 lanes per packet");
template <bool OPEN, bool RX = false>
__global__ __launch_bounds__(kTailWaves * kWave) void gcm_single_tail_kernel(GcmArgs args) {
    __shared__ TailLds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t npkt = args.npkt;
    if (args.npkt_dev) npkt = min(npkt, __builtin_amdgcn_readfirstlane(*args.npkt_dev));
    const uint32_t ngroups = (npkt + kPpw - 1u) / kPpw, slots = args.tail_slots;
    uint32_t p0 = 0;  // kTailAll: a small batch, every packet here
    if (slots != kTailAll) {
        if (ngroups <= slots || ngroups % slots == 0u) return;  // no partial pass: nothing to do
        p0 = ngroups / slots * slots * kPpw;
    }
    const uint32_t tgroups = (npkt - p0 + kTailPpw - 1u) / kTailPpw;
    if (blockIdx.x * kTailWaves >= tgroups) return;
    const uint32_t* srec = args.keys + (size_t)args.key_hint * kKeyRecDwords;
    fill_ttab<256u * 32u, kTailWaves * kWave>(lds.ttab, tid, ttab_entry);
    stage_gh64(lds.gh, srec, tid, kTailWaves * kWave);
    uint32_t rks[60];
    load_round_keys(srec, rks);
    __syncthreads();
    const TLook T{lds.ttab, ttab_lane_base(lane)};
    const GhShoup64 gh{&lds.gh};
    const bool key_ok = __builtin_amdgcn_readfirstlane(srec[kRecAlg]) == NEB_ALG_AESGCM;
    for (uint32_t t = blockIdx.x * kTailWaves + wave; t < tgroups; t += gridDim.x * kTailWaves) {
        const uint32_t p = p0 + kTailPpw * t + (lane >> kTailLg);
        gcm_packet_group<OPEN, false, RX>(args, p, p < npkt, args.key_hint, key_ok, RkRegs{rks}, gh, T, lane, kTailLg);
    }
}

// ---- one packet, its bytes in the kernel arguments (the per-packet CipherState calls) ---------
// A per-packet call through the tail kernel spent ≈ 18.6 µs on the device for one packet, mostly
// a chain of PCIe round trips to the caller's pinned staging: the descriptor, then each round's
// payload block, then (open) the received tag. Here the host puts the descriptor, the AAD and the
// payload (+ tag) into the kernel's argument block, which the runtime writes to device memory with
// the dispatch, so the kernel reads nothing over PCIe; it writes the result and the status into
// the caller's pinned staging (posted writes). One wave, 64 lanes per packet (2 rounds for 1300 B).
// The block holds kOneBytes of packet (cipher.hpp).

// The status goes out last, behind a system-scope release of the wave's result stores, so the host
// may take the result as soon as it sees the status word change (engine.cpp one_packet) instead of
// waiting for the stream (hipStreamSynchronize: ≈ 26 µs of a ≈ 36 µs call, round 4).
struct OneArgs {
    neb_desc d;           // offsets from `in`; dst_off reaches the host output (a wrapping 64-bit offset)
    const uint32_t* keys;
    uint32_t max_keys, key;
    int32_t* status;      // host
    uint32_t pad_[2];
    uint8_t in[kOneBytes];  // 16-B aligned within the argument block
};
static_assert(offsetof(OneArgs, in) % 16 == 0, "the packet bytes are read as 16-B blocks");
// The 64 KiB T-table image is filled by NEB_ONE_FILL_WAVES waves (the packet's one wave alone spent
// most of the kernel on it); the others leave after the fill.
#ifndef NEB_ONE_FILL_WAVES
#define NEB_ONE_FILL_WAVES 4
#endif
constexpr uint32_t kOneFillThreads = NEB_ONE_FILL_WAVES * kWave;
template <bool OPEN>
__global__ __launch_bounds__(kOneFillThreads) void gcm_one_kernel(OneArgs a) {
    __shared__ TailLds lds;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1u);
    // the argument block in place (a by-value struct indexed per lane would be copied to scratch)
    // the block's address as an opaque integer: derived from the constant-address kernarg pointer,
    // the output address (base + dst_off) would let the compiler treat the result stores as stores
    // to constant memory and drop them
    OneTrace ot;
    ot.kernel_begin();
    uint64_t kb = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kb));
    const uint8_t* ka = reinterpret_cast<const uint8_t*>(kb);
    const uint32_t key = a.key;
    const uint32_t* srec = a.keys + (size_t)(key < a.max_keys ? key : 0u) * kKeyRecDwords;
    // The packet's bytes (the argument block's 2 KiB, in device memory) are touched by the fill's
    // threads first, so the rounds' block loads after the fill hit the caches (0.4 µs of 12).
    uint4 warm = make_uint4(0, 0, 0, 0);
    if (tid < kOneBytes / 16u) warm = *reinterpret_cast<const uint4*>(ka + offsetof(OneArgs, in) + 16u * tid);
    // T-tables, 16 entries per thread at a time (loads before stores, as fill_ttab)
    for (uint32_t j0 = 0; j0 < 256u * 32u; j0 += 16u * kOneFillThreads) {
        uint2 v[16];
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++) v[j] = ttab_entry(j0 + j * kOneFillThreads + tid);
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++) lds.ttab[j0 + j * kOneFillThreads + tid] = v[j];
    }
    stage_gh64(lds.gh, srec, tid, kOneFillThreads);
    asm volatile("" ::"v"(warm.x), "v"(warm.y), "v"(warm.z), "v"(warm.w));  // the loads complete
    __syncthreads();
    if (tid >= kWave) return;  // the packet is one wave's
    ot.filled();
    uint32_t rks[60];
    load_round_keys(srec, rks);
    const TLook T{lds.ttab, ttab_lane_base(lane)};
    const GhShoup64 gh{&lds.gh};
    const bool key_ok = key < a.max_keys && __builtin_amdgcn_readfirstlane(srec[kRecAlg]) == NEB_ALG_AESGCM;
    uint8_t* base = const_cast<uint8_t*>(ka + offsetof(OneArgs, in));
    __shared__ int32_t s_status;
    GcmArgs ga{nullptr, 1u, base, a.keys, a.max_keys, key, &s_status, nullptr, 0u, 0u, nullptr};
    // the host passed the output's address in dst_off: rebase it on the argument block (wrapping)
    neb_desc d = a.d;
    d.dst_off = a.d.dst_off - (uint64_t)(uintptr_t)base;
    ot.keyed();
    gcm_packet_group<OPEN>(ga, 0u, true, key, key_ok, RkRegs{rks}, gh, T, lane, kTailLg, nullptr, &d);
    one_publish_status(a.status, &s_status);
    ot.done(lane, OPEN);
}

// ---- per-packet calls that arrive together, in one launch (engine.cpp's combiner) -------------
// Concurrent EncryptDanger / DecryptDanger calls (several threads, each its own tunnel) that arrive
// while another call's launch is being made are collected in a pinned batch buffer and launched
// together: one wave per request, four waves per workgroup. The waves fill the workgroup's T-table
// image together; each stages its own key's GHASH tables (the per-packet kernel's set, GhShoup64)
// in a slice of its own and copies its request's slot from host memory into LDS with one parallel
// load (under the fill), then seals or opens it at 64 lanes, writes the result back into its slot
// (in place, host memory) and publishes its status last (one_publish_status), as the per-packet
// kernel does. The buffer (engine.cpp PktComb): statuses and slots (request r's bytes in slot r,
// kCombSlot apart); the descriptors (offsets from the slots' base) travel in the kernel arguments,
// so the key record's loads do not wait for a PCIe round trip (17.5 µs per launch with the
// descriptors in the pinned buffer, round-6 trace).
constexpr int kOneBatchWaves = 4;
struct OneBatchDescs {
    neb_desc d[kCombMax];
};
struct OneBatchLds {
    uint2 ttab[256 * 32];  // 64 KiB T-table pairs, 32 copies
    Gh64Tabs k[kOneBatchWaves];                       // each wave's key
    uint4 data[kOneBatchWaves][kCombSlot / 16u];      // the request's slot
    int32_t st[kOneBatchWaves];
};
template <bool OPEN>
__global__ __launch_bounds__(kOneBatchWaves * kWave) void gcm_one_batch_kernel(const OneBatchDescs descs, int32_t* status,
                                                                                uint8_t* slots, uint32_t n,
                                                                                const uint32_t* keys,
                                                                                uint32_t max_keys) {
    __shared__ OneBatchLds lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t r = blockIdx.x * kOneBatchWaves + w;
    const bool have = r < n;
    // the request's descriptor and bytes first (host memory: one PCIe round trip, under the fill)
    constexpr uint32_t kSlotVecs = kCombSlot / 16u;
    neb_desc d = {};
    uint4 b[(kSlotVecs + kWave - 1) / kWave];
    if (have) {
        d = descs.d[r];
#pragma unroll
        for (uint32_t k = 0; k < (kSlotVecs + kWave - 1) / kWave; k++)
            if (k * kWave + lane < kSlotVecs)
                b[k] = *reinterpret_cast<const uint4*>(slots + (size_t)r * kCombSlot + 16u * (k * kWave + lane));
    }
    fill_ttab<256u * 32u, kOneBatchWaves * kWave>(lds.ttab, tid, ttab_entry);
    const uint32_t key = __builtin_amdgcn_readfirstlane(d.key_id);
    const uint32_t* srec = keys + (size_t)(key < max_keys ? key : 0u) * kKeyRecDwords;
    Gh64Tabs& kt = lds.k[w];
    if (have) {
        stage_gh64(kt, srec, lane, kWave);
#pragma unroll
        for (uint32_t k = 0; k < (kSlotVecs + kWave - 1) / kWave; k++)
            if (k * kWave + lane < kSlotVecs) lds.data[w][k * kWave + lane] = b[k];
    }
    __syncthreads();
    if (!have) return;
    uint32_t rks[60];
    load_round_keys(srec, rks);
    const TLook T{lds.ttab, ttab_lane_base(lane)};
    const GhShoup64 gh{&kt};
    const bool key_ok = key < max_keys && __builtin_amdgcn_readfirstlane(srec[kRecAlg]) == NEB_ALG_AESGCM;
    // the bytes in LDS, addressed through a generic pointer (flat loads): the descriptor's offsets are
    // from the slots' base, so the LDS copy stands at slot r's place; the output goes to the slot in
    // host memory (a wrapping offset from there)
    uint64_t lb = (uint64_t)(uintptr_t)(const void*)&lds.data[w][0] - (uint64_t)r * kCombSlot;
    asm volatile("" : "+s"(lb));
    uint8_t* base = reinterpret_cast<uint8_t*>(lb);
    d.dst_off = d.dst_off + (uint64_t)(uintptr_t)slots - lb;
    GcmArgs ga{nullptr, 1u, base, keys, max_keys, key, &lds.st[w], nullptr, 0u, 0u, nullptr};
    gcm_packet_group<OPEN>(ga, 0u, true, key, key_ok, RkRegs{rks}, gh, T, lane, kTailLg, nullptr, &d);
    one_publish_status(status + r, &lds.st[w]);
}

// ---- mixed keys: one key per chunk of the regrouped batch (sched.hpp) --------------------------


// One kernel, two code paths, each specialised for its chunk shape (one path with a run-time lanes
// per packet spilled 52-64 B per lane at 128 VGPRs, inside the chunk loop):
//  front chunks (chunks[0, F)): groups of 16 packets at 4 lanes each, the layout of the single-key
//               kernel (GhChunk4), one after another on one staging of the key;
//  back chunks (chunks[max - 1 - j], j < B): tails of 1-8 packets at 8 or 16 lanes (GhChunkTail).
// The two-table AES (64 KiB): 16 waves per workgroup, one workgroup per CU.
constexpr int kChunkWaves = 16;
constexpr int kChunkWpe = 4;  // launch bound: waves per SIMD (at most 128 VGPRs)
constexpr int kChunkThreads = kChunkWaves * kWave;

struct ChunkLds {
    uint4 shoup[kChunkWaves][5][16];  // per wave: Shoup tables (1.25 KiB): M_1..M_4, and M_8 (tails)
    uint4 pos[kChunkWaves][8 * 16];   // per wave: position tables of H^(2^lg) (2 KiB)
    uint2 ttab[256 * 32];             // 64 KiB T-table pairs, 32 copies
};

// Stage a chunk key's GHASH tables in the wave's LDS slice, computed from the record's raw powers
// H^1..H^16 (16 B each) rather than copied from its precomputed tables: 128 B of key material per
// chunk instead of 3 KiB, which for IMIX-sized chunks was a third of the kernel's memory traffic.
//   shoup[t][v] = v·H^(t+1), t < 4, and (tails) shoup[4][v] = v·H^8
//   pos[r][v]   = v·x^(4r)·P, r < 8, P = H^(2^lg): XOR of the basis P·x^(4r+j) over the set bits
//                 of v (bit 3 ↔ j = 0), the basis P·x^i (i < 32) one per lane and shuffled
template <bool FULL>
__device__ __forceinline__ void stage_chunk_tables(const uint32_t* rec, uint32_t lane, uint32_t lg, uint4* wtab,
                                                   uint4* wpos) {
    const uint32_t t = lane >> 4, v = lane & 15u;
    const uint4 he = ld_rec4(rec, kRecHPow + 4u * t);
    const uint4 P = ld_rec4(rec, kRecHPow + 4u * ((1u << lg) - 1u));
    wtab[lane] = gf_tab_entry(he, v);
    if constexpr (!FULL) {
        const uint4 h8 = ld_rec4(rec, kRecHPow + 4u * 7u);
        if (lane < 16u) wtab[64u + lane] = gf_tab_entry(h8, v);
    }
    const uint4 B = gf_mul_xpow32(P, lane & 31u);
    uint4 e0 = make_uint4(0, 0, 0, 0), e1 = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint4 b0 = shfl4(B, 4u * t + j), b1 = shfl4(B, 4u * t + 16u + j);
        const uint32_t m = (v >> (3u - j)) & 1u ? ~0u : 0u;
        e0 = xor4(e0, make_uint4(b0.x & m, b0.y & m, b0.z & m, b0.w & m));
        e1 = xor4(e1, make_uint4(b1.x & m, b1.y & m, b1.z & m, b1.w & m));
    }
    wpos[lane] = e0;
    wpos[64u + lane] = e1;
}

struct ChunkArgs {
    const uint32_t* sorted;
    const uint4* chunks;  // [kBuckets][max_chunks] (sched.hpp)
    uint32_t* counters;   // the scheduler's counters (sched.hpp kCnt*)
    uint32_t max_chunks;
};

// Chunk order: the cost buckets in turn, longest first (sched.hpp sched_bucket). Workgroup w owns
// chunks w, w + G, w + 2G, ... of that order (G workgroups) and its waves draw them from an LDS
// cursor as each finishes its chunk. Balance stays dynamic inside the workgroup and no wave touches a global atomic (a global work cursor: returning
// atomics on one word serialise across the chip; C3 step -8%, IMIX -27% against it, A/B,
// profiles/r2_micro/ab_chunk_order.log).
template <bool OPEN, bool RX = false>
__global__ __launch_bounds__(kChunkThreads, kChunkWpe) void gcm_chunk_kernel(GcmArgs args, ChunkArgs ca) {
    __shared__ ChunkLds lds;
    __shared__ uint32_t wg_cursor;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    // chunk index space: bucket 0's chunks, then bucket 1's, ... (bucket b's records from b * max_chunks);
    // the buckets' ends in LDS (read per chunk: held in registers they were spilled)
    __shared__ uint32_t s_bend[kBuckets];
    uint32_t nch = 0;
#pragma unroll
    for (uint32_t b = 0; b < kBuckets; b++) nch += min(__builtin_amdgcn_readfirstlane(ca.counters[kCntBucket + b]), ca.max_chunks);
    if (tid < kBuckets) {
        uint32_t e = 0;
        for (uint32_t b = 0; b <= tid; b++) e += min(ca.counters[kCntBucket + b], ca.max_chunks);
        s_bend[tid] = e;
    }
    if (blockIdx.x >= nch) return;  // owns no chunk (uniform over the workgroup)
    WaveTimeline wt;
    wt.kernel_begin(wave);
    fill_ttab<256u * 32u, kChunkThreads>(lds.ttab, tid, ttab_entry);
    if (tid == 0) wg_cursor = kChunkWaves;
    __syncthreads();
    wt.tables_filled(lane);
    uint4* wtab = &lds.shoup[wave][0][0];
    uint4* wpos = &lds.pos[wave][0];
    auto chunk_at = [&](uint32_t c) {
        uint32_t b = 0, lo = 0;
        for (uint32_t k = 0; k + 1u < kBuckets; k++) {
            const uint32_t e = __builtin_amdgcn_readfirstlane(s_bend[k]);
            if (c < e) break;
            b = k + 1u;
            lo = e;
        }
        return ca.chunks[(size_t)b * ca.max_chunks + (c - lo)];
    };
    // Workgroup w owns chunks w, w + G, w + 2G, ... (the longest first) and its waves
    // draw them from an LDS cursor as they finish. Drawing the last 10-50% from a global cursor
    // instead (dynamic balance across workgroups) made the C3 kernel 26-50% slower: the returning
    // atomics on one word serialise across the chip (A/B).
    auto chunk_of = [&](uint32_t k) -> uint32_t { return blockIdx.x + k * gridDim.x; };
    uint32_t c = 0;
    if (lane == 0u) c = chunk_of(wave);
    c = __builtin_amdgcn_readfirstlane(c);
    uint4 ch_next = make_uint4(0, 0, 0, 0);
    if (c < nch) ch_next = chunk_at(c);
#ifndef NEB_STEAL_MIN_PER_WG
#define NEB_STEAL_MIN_PER_WG 32u
#endif
    // The batch's last 1/8 of chunks (the shortest) are not owned: a wave whose workgroup has run
    // out of its own draws them from its XCD's cursor (blockIdx mod 8, one word per XCD, 128 B
    // apart), so workgroups that drew lighter chunks take more of them. C5's workgroups carried
    // 3752-4426 packets and spanned 562-616 µs with every chunk owned (tools/wave_trace.py). A/B,
    // alternating (profiles/r5/ab_balance): C3 547-548 -> 553-555 GiB/s, C5 512-514 -> 518; the
    // last 1/4 or 1/16 the same within noise. Every partition has a drawer (at least 8 workgroups)
    // and every wave's first chunk is still owned (at least 32 chunks per workgroup).
    const uint32_t ndyn = (gridDim.x >= 8u && nch >= NEB_STEAL_MIN_PER_WG * gridDim.x) ? nch / NEB_CHUNK_STEAL : 0u;
    const uint32_t nstat = nch - ndyn;
    auto claim = [&]() -> uint32_t {
        uint32_t k = 0;
        if (lane == 0u) {
            k = chunk_of(atomicAdd(&wg_cursor, 1u));
            if (k >= nstat) {
                const uint32_t x = blockIdx.x & 7u;
                k = nstat + x + 8u * atomicAdd(&ca.counters[kCntSteal + kStealStride * x], 1u);
            }
        }
        return __builtin_amdgcn_readfirstlane(k);
    };
    while (c < nch) {
        const uint4 ch = ch_next;
        NEB_MARK(chunk_begin);
        const uint32_t cw = __builtin_amdgcn_readfirstlane(ch.w);
        const bool full = (cw >> 20) & 1u;  // 4-lane groups (front), or one group at 8 or 16 lanes
        wt.chunk_begin();
        // Lane-derived constants (the T-table lane base, shuffle sources, the final's permutation)
        // are rebuilt per chunk from an opaque copy of the lane index: hoisted out of the chunk loop
        // they stay live across it and the compiler spills them (36-104 B of scratch per lane).
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));
        const TLook T{lds.ttab, ttab_lane_base(ln)};
        wt.phases_begin(lane);  // the chunk's descriptor in
        // the chunk's packets: segment 0 (count0 from start0 in sorted), then segment 1 (a smaller
        // class's leftover packets riding in free slots, sched_key_chunks)
        const uint32_t start = __builtin_amdgcn_readfirstlane(ch.x);
        const uint32_t start1 = __builtin_amdgcn_readfirstlane(ch.y);
        const uint32_t count0 = cw & 0xFFu, count = count0 + ((cw >> 8) & 0xFFu);
        const uint32_t key = __builtin_amdgcn_readfirstlane(ch.z);
        auto sorted_at = [&](uint32_t q) { return ca.sorted[q < count0 ? start + q : start1 + (q - count0)]; };
        const uint32_t* rec = args.keys + (size_t)(key < args.max_keys ? key : 0u) * kKeyRecDwords;
        const bool key_ok = key < args.max_keys && rec[kRecAlg] == NEB_ALG_AESGCM;
        uint32_t rks[60];
        load_round_keys(rec, rks);
        wt.keys_in();
        if (full) {
            NEB_MARK(stage_full);
            stage_chunk_tables<true>(rec, ln, 2u, wtab, wpos);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            wt.tables_staged();
            // the chunk's groups of 16 packets at 4 lanes, one after another on the staged tables
            const GhChunk4 gh{wtab, wpos};
            for (uint32_t g0 = 0; g0 < count; g0 += kChunkPkts) {
                const uint32_t q = g0 + (ln >> 2);
                const uint32_t sp = q < count ? sorted_at(q) : kSortedSkip;
                const bool valid = sp != kSortedSkip;  // (a device receive's refused packet: skipped)
                const uint32_t p = valid ? sp : 0u;
                gcm_packet_group<OPEN, false, RX>(args, p, valid, key, key_ok, RkRegs{rks}, gh, T, ln, 2u);
            }
        } else {
            const uint32_t lg = (cw >> kChunkLgShift) & 15u;  // 3 or 4
            NEB_MARK(stage_tail);
            stage_chunk_tables<false>(rec, ln, lg, wtab, wpos);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            wt.tables_staged();
            const uint32_t q = ln >> lg;
            const uint32_t sp = q < count ? sorted_at(q) : kSortedSkip;
            const bool valid = sp != kSortedSkip;
            const uint32_t p = valid ? sp : 0u;
            const GhChunkTail gh{wtab, wpos};
            gcm_packet_group<OPEN, false, RX>(args, p, valid, key, key_ok, RkRegs{rks}, gh, T, ln, lg);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the slice is rewritten next chunk
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the next chunk is claimed when this one is done, not when it starts: a claim at the start
        // handed the workgroup's second round of chunks to whichever waves reached the cursor first
        // at time 0 (the older ones), and C3's waves then finished 97-115 µs apart
        // (tools/wave_trace.py). A/B, alternating (profiles/r5/ab_balance): C3 526-527 -> 536-537 GiB/s,
        // C5 504-505 -> 515-516; claiming ahead only while more than a round of chunks is left:
        // C3 537-542, C5 506-508.
        NEB_MARK(chunk_claim);
        const uint32_t cn = claim();
        if (cn < nch) ch_next = chunk_at(cn);
        NEB_MARK(chunk_claimed);
        wt.chunk_end(lane, min(count, 255u) << 8 | ((cw >> kChunkLgShift) & 15u) << 4 | (full ? 1u : 0u), c);
        wt.phases_end(lane);
        c = cn;
    }
}

// ------------------------------------------------------------------------------------------
// Key install: AES-256 key expansion, H = E_K(0), H^1..H^16, and the GHASH tables.
// Runs once per tunnel key (one workgroup of 256 lanes).

__device__ uint8_t sbox_b(uint32_t x) { return (uint8_t)(c_T0.t[x & 255u] >> 8); }
__device__ uint8_t xtime_d(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }

// One workgroup per key of a batch install (neb_cipher_create_batch: n keys in one launch); the
// workgroup first clears its record (the slot may have held another key or algorithm).
__global__ __launch_bounds__(256) void gcm_key_setup_kernel(const uint8_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ slots,
                                                            uint32_t* __restrict__ table) {
    const uint8_t* key = keys + 32u * blockIdx.x;
    uint32_t* rec = table + (size_t)slots[blockIdx.x] * kKeyRecDwords;
    for (uint32_t j = threadIdx.x; j < kKeyRecDwords; j += blockDim.x) rec[j] = 0u;
    __shared__ uint4 hp[16];      // H^1..H^16
    __shared__ uint4 basis[128];  // x^i · H^kFullPow
    __shared__ uint4 basis8[32];  // x^i · H^8
    __shared__ uint4 basis16[32]; // x^i · H^16
    __shared__ uint4 basis23[2][32]; // x^i · H^2, x^i · H^3
    __shared__ uint4 basis12[32];    // x^i · H^12
    __shared__ uint4 basis_h[128];  // x^i · H
    __shared__ uint4 part[2];
    // the S-box in LDS for the key schedule and H = E_K(0) on lane 0: its ~330 dependent lookups
    // from global memory cost ~25 µs per key
    __shared__ uint8_t sb[256];
    __shared__ uint8_t rk[240];  // the key schedule (in LDS: as a lane array it lived in scratch)
    sb[threadIdx.x] = (uint8_t)(c_T0.t[threadIdx.x] >> 8);
    __syncthreads();
    if (threadIdx.x == 0) {
        auto sbox_b = [&](uint32_t x) { return sb[x & 255u]; };
        for (int i = 0; i < 32; i++) rk[i] = key[i];
        uint8_t rcon = 1;
        for (int i = 8; i < 60; i++) {
            uint8_t t0 = rk[4 * i - 4], t1 = rk[4 * i - 3], t2 = rk[4 * i - 2], t3 = rk[4 * i - 1];
            if (i % 8 == 0) {
                uint8_t u = t0;
                t0 = sbox_b(t1) ^ rcon; t1 = sbox_b(t2); t2 = sbox_b(t3); t3 = sbox_b(u);
                rcon = xtime_d(rcon);
            } else if (i % 8 == 4) {
                t0 = sbox_b(t0); t1 = sbox_b(t1); t2 = sbox_b(t2); t3 = sbox_b(t3);
            }
            rk[4 * i] = rk[4 * i - 32] ^ t0; rk[4 * i + 1] = rk[4 * i - 31] ^ t1;
            rk[4 * i + 2] = rk[4 * i - 30] ^ t2; rk[4 * i + 3] = rk[4 * i - 29] ^ t3;
        }
        for (int i = 0; i < 60; i++)
            rec[kRecRoundKeys + i] = (uint32_t)rk[4 * i] | (uint32_t)rk[4 * i + 1] << 8 |
                                     (uint32_t)rk[4 * i + 2] << 16 | (uint32_t)rk[4 * i + 3] << 24;
        // H = E_K(0^128), byte-oriented FIPS-197 cipher
        uint8_t s[16];
        for (int i = 0; i < 16; i++) s[i] = rk[i];
        for (int r = 1; r <= 14; r++) {
            uint8_t t[16];
            for (int c = 0; c < 4; c++)
                for (int j = 0; j < 4; j++) t[4 * c + j] = sbox_b(s[4 * ((c + j) & 3) + j]);
            if (r != 14) {
                for (int c = 0; c < 4; c++) {
                    uint8_t a0 = t[4 * c], a1 = t[4 * c + 1], a2 = t[4 * c + 2], a3 = t[4 * c + 3];
                    uint8_t x = a0 ^ a1 ^ a2 ^ a3;
                    t[4 * c] = a0 ^ x ^ xtime_d(a0 ^ a1);
                    t[4 * c + 1] = a1 ^ x ^ xtime_d(a1 ^ a2);
                    t[4 * c + 2] = a2 ^ x ^ xtime_d(a2 ^ a3);
                    t[4 * c + 3] = a3 ^ x ^ xtime_d(a3 ^ a0);
                }
            }
            for (int i = 0; i < 16; i++) s[i] = t[i] ^ rk[16 * r + i];
        }
        uint32_t h[4];
        for (int i = 0; i < 4; i++)
            h[i] = (uint32_t)s[4 * i] << 24 | (uint32_t)s[4 * i + 1] << 16 | (uint32_t)s[4 * i + 2] << 8 | s[4 * i + 3];
        hp[0] = make_uint4(h[0], h[1], h[2], h[3]);
    }
    __syncthreads();
    // basis_h[i] = x^i·H: a product P·H is the XOR of basis_h[i] over the set bits i of P
    if (threadIdx.x < 128u) basis_h[threadIdx.x] = gf_mul_xpow(hp[0], threadIdx.x);
    __syncthreads();
    // H^2..H^16: H^k = H^(k-1)·H with lane i < 128 contributing basis_h[i] if bit i of H^(k-1) is
    // set, XOR-reduced across the two waves (the bit-serial form on one lane took ~100 µs).
    for (uint32_t k = 1; k < kNumHPow; k++) {
        const uint32_t t = threadIdx.x;
        const uint4 P = hp[k - 1];
        uint4 c = make_uint4(0, 0, 0, 0);
        if (t < 128u) {
            const uint32_t w = t < 32u ? P.x : (t < 64u ? P.y : (t < 96u ? P.z : P.w));
            if ((w >> (31u - (t & 31u))) & 1u) c = basis_h[t];
        }
        for (int m = 32; m >= 1; m >>= 1) c = xor4(c, shfl_xor4(c, m));
        if (t == 0u || t == 64u) part[t >> 6] = c;
        __syncthreads();
        if (t == 0u) hp[k] = xor4(part[0], part[1]);
        __syncthreads();
    }
    if (threadIdx.x < 64u) {
        const uint4 v = hp[threadIdx.x >> 2];
        const uint32_t c = threadIdx.x & 3u;
        rec[kRecHPow + threadIdx.x] = c == 0u ? v.x : c == 1u ? v.y : c == 2u ? v.z : v.w;
    }
    if (threadIdx.x < 128u) basis[threadIdx.x] = gf_mul_xpow(hp[kFullPow - 1], threadIdx.x);
    if (threadIdx.x < 32u) {
        basis8[threadIdx.x] = gf_mul_xpow(hp[7], threadIdx.x);
        basis16[threadIdx.x] = gf_mul_xpow(hp[15], threadIdx.x);
        basis23[0][threadIdx.x] = gf_mul_xpow(hp[1], threadIdx.x);
        basis23[1][threadIdx.x] = gf_mul_xpow(hp[2], threadIdx.x);
        basis12[threadIdx.x] = gf_mul_xpow(hp[11], threadIdx.x);
    }
    if (threadIdx.x == 0) rec[kRecAlg] = NEB_ALG_AESGCM;
    __syncthreads();
    const uint32_t t = threadIdx.x;
    // Shoup tables: entry (k, v) for k = 1..16
    {
        const uint32_t k = t >> 4, v = t & 15u;
        const uint4 e = gf_tab_entry(hp[k], v);
        uint32_t* o = rec + kRecShoup + 64u * k + 4u * v;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    // full table of H^kFullPow: F_p[v] = XOR of basis[4p + j] for the set bits of v (bit 3 ↔ j = 0)
    for (uint32_t i = t; i < 512u; i += 256u) {
        const uint32_t p = i >> 4, v = i & 15u;
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 0; j < 4; j++)
            if ((v >> (3 - j)) & 1u) e = xor4(e, basis[4 * p + j]);
        uint32_t* o = rec + kRecFull + 4u * i;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    // position tables of H^8 and H^16: T_r[v] = XOR of basis[4r + j] for the set bits of v
    {
        const uint32_t tab = t >> 7, i = t & 127u, r = i >> 4, v = i & 15u;
        const uint4* bs = tab ? basis16 : basis8;
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 0; j < 4; j++)
            if ((v >> (3 - j)) & 1u) e = xor4(e, bs[4 * r + j]);
        uint32_t* o = rec + (tab ? kRecPos16 : kRecPos8) + 4u * i;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    if (t < 128u) {  // and of H
        const uint32_t r = t >> 4, v = t & 15u;
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 0; j < 4; j++)
            if ((v >> (3 - j)) & 1u) e = xor4(e, basis_h[4 * r + j]);
        uint32_t* o = rec + kRecPos1 + 4u * t;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    if (t < 128u) {  // and of H^12
        const uint32_t r = t >> 4, v = t & 15u;
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 0; j < 4; j++)
            if ((v >> (3 - j)) & 1u) e = xor4(e, basis12[4 * r + j]);
        uint32_t* o = rec + kRecPos12 + 4u * t;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    {  // and of H^2, H^3
        const uint32_t tab = t >> 7, i = t & 127u, r = i >> 4, v = i & 15u;
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 0; j < 4; j++)
            if ((v >> (3 - j)) & 1u) e = xor4(e, basis23[tab][4 * r + j]);
        uint32_t* o = rec + (tab ? kRecPos3 : kRecPos2) + 4u * i;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    // H^32 .. H^512 by squaring (the tail kernel's 64-lane packets, the TX seal's checksum
    // correction): P·Q is the XOR of basis[i] = x^i·Q over the set bits i of P (lane i < 128), as
    // for H^2..H^16 above
    auto basis_of = [&](uint4 q, uint32_t cnt) {
        __syncthreads();  // basis[] is free again
        if (t < cnt) basis[t] = gf_mul_xpow(q, t);
        __syncthreads();
    };
    auto mul_by_basis = [&](uint4 P) -> uint4 {
        uint4 c = make_uint4(0, 0, 0, 0);
        if (t < 128u) {
            const uint32_t w = t < 32u ? P.x : (t < 64u ? P.y : (t < 96u ? P.z : P.w));
            if ((w >> (31u - (t & 31u))) & 1u) c = basis[t];
        }
        for (int m = 32; m >= 1; m >>= 1) c = xor4(c, shfl_xor4(c, m));
        if (t == 0u || t == 64u) part[t >> 6] = c;
        __syncthreads();
        const uint4 r = xor4(part[0], part[1]);
        __syncthreads();
        return r;
    };
    basis_of(hp[15], 128u);
    const uint4 h32 = mul_by_basis(hp[15]);
    const uint4 h48 = mul_by_basis(h32);  // (the basis is still H^16's)
    basis_of(h32, 128u);
    const uint4 h64 = mul_by_basis(h32);
    basis_of(h64, 128u);
    const uint4 h128 = mul_by_basis(h64);
    if (t < 128u) {  // the position tables of H^64 (basis[0, 32))
        const uint32_t r = t >> 4, v = t & 15u;
        uint4 e = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 0; j < 4; j++)
            if ((v >> (3 - j)) & 1u) e = xor4(e, basis[4 * r + j]);
        uint32_t* o = rec + kRecPos64 + 4u * t;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
    basis_of(h128, 128u);
    const uint4 h256 = mul_by_basis(h128);
    basis_of(h256, 128u);
    const uint4 h512 = mul_by_basis(h256);
    if (t < 96u) {  // Shoup tables of H^32, H^64, H^128, H^256, H^512 and H^48
        const uint32_t k = t >> 4, v = t & 15u;
        const uint4 P = k == 0u ? h32 : k == 1u ? h64 : k == 2u ? h128 : k == 3u ? h256 : k == 4u ? h512 : h48;
        const uint4 e = gf_tab_entry(P, v);
        uint32_t* o = rec + (k < 5u ? rec_shoup_pow2(5u + k) : kRecShoup48) + 4u * v;
        o[0] = e.x; o[1] = e.y; o[2] = e.z; o[3] = e.w;
    }
}

}  // namespace neb

// ------------------------------------------------------------------------------------------
// Host-side launchers (called by engine.cpp)

extern "C" hipError_t neb_gcm_probe(void) {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, (const void*)neb::gcm_single_kernel<false>);
}

extern "C" hipError_t neb_gcm_key_setup(const uint8_t* keys, const uint32_t* slots, uint32_t n, uint32_t* table,
                                        hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(neb::gcm_key_setup_kernel, dim3(n), dim3(256), 0, s, keys, slots, table);
    return hipGetLastError();
}

// Launch over min(workgroups the work needs, what the device holds at once) with `stop` (optional)
// bound to the dispatch (hipExtLaunchKernel): the event completes with the kernel, and no marker
// packet follows it on the stream
constexpr int kMaxDevices = 64;
template <class K, class... Extra>
static hipError_t launch_grid_stop(K kern, int threads, uint32_t work_waves, int cu_count, hipStream_t s,
                                   hipEvent_t stop, Extra... args) {
    // workgroups per CU, cached per instantiation and device (engines on GPUs of different
    // architectures in one process each get their own)
    static std::atomic<int> cache[kMaxDevices];
    int dev = 0;
    (void)hipGetDevice(&dev);
    int per_cu = dev >= 0 && dev < kMaxDevices ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (per_cu < 1) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, 0) != hipSuccess || per_cu < 1)
            per_cu = 1;
        if (dev >= 0 && dev < kMaxDevices) cache[dev].store(per_cu, std::memory_order_relaxed);
    }
    const uint32_t waves = (uint32_t)threads / 64u;
    const uint32_t want = (work_waves + waves - 1) / waves;
    const uint32_t cap = (uint32_t)(per_cu * cu_count);
    const uint32_t grid = want < cap ? want : cap;
    if (grid == 0) return stop ? hipEventRecord(stop, s) : hipSuccess;
    return neb::launch_bound(kern, dim3(grid), dim3(threads), s, stop, args...);
}

// ---- one tunnel key (key_hint) for every descriptor --------------------------------------------

// The instantiations by batch kind: cs = the TX seal with its checksums (tx.hip), rx = the device
// receive's open (an admission mask)
using GcmKernel = void (*)(neb::GcmArgs);
static GcmKernel single_kernel_of(bool open, bool cs, bool rx) {
    if (open) return rx ? neb::gcm_single_kernel<true, false, true> : neb::gcm_single_kernel<true>;
    return cs ? neb::gcm_single_kernel<false, true> : neb::gcm_single_kernel<false>;
}
static GcmKernel tail_kernel_of(bool open, bool rx) {
    if (open) return rx ? neb::gcm_single_tail_kernel<true, true> : neb::gcm_single_tail_kernel<true>;
    return neb::gcm_single_tail_kernel<false>;
}

// Waves of gcm_single_kernel's grid for a batch of at most n packets (a full pass is that many
// groups of kPpw packets; the packets after the last full pass go to the tail kernel). The TX
// segment kernel uses it to know which segments the tail seals (without the checksum).
extern "C" uint32_t neb_gcm_single_slots(uint32_t n, int cu_count, int open, int hdr_from_dst) {
    const uint32_t groups = (n + neb::kPpw - 1u) / neb::kPpw;
    const void* kern = (const void*)single_kernel_of(open, !open && hdr_from_dst == 2, false);
    int per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, neb::kSingleThreads, 0) != hipSuccess || per_cu < 1)
        per_cu = 1;
    uint32_t cap = (uint32_t)(per_cu * cu_count);
    // test hook: a smaller grid, so that small batches have a partial last pass (the tail kernel)
    if (const int64_t g = neb::knob(NEB_KNOB_SINGLE_MAX_GRID); g > 0) cap = std::max(1u, std::min<uint32_t>(cap, (uint32_t)g));
    // one workgroup per group up to the cap: a small batch runs one or a few groups per CU
    const uint32_t grid = std::min(groups, cap);
    return grid * neb::kSingleWaves;
}

// The tail kernel over up to `pkts` packets. The grid is capped at two workgroups per CU (as many as
// fit; the kernel strides over the rest): one workgroup per possible tail wave put 8 Ki mostly empty
// workgroups behind every TX batch (a 29-packet tail took 20 µs, almost all of it dispatching
// workgroups that exit).
static hipError_t launch_tail(bool open, bool rx, uint32_t pkts, int cu_count, hipStream_t s, hipEvent_t stop,
                              const neb::GcmArgs& a) {
    const uint32_t tgrid = std::min<uint32_t>(
        ((pkts + neb::kTailPpw - 1u) / neb::kTailPpw + neb::kTailWaves - 1u) / neb::kTailWaves,
        2u * (uint32_t)std::max(cu_count, 1));
    (void)neb::launch_bound(tail_kernel_of(open, rx), dim3(tgrid), dim3(neb::kTailWaves * neb::kWave), s, stop, a);
    return hipGetLastError();
}

// Launch on s; `stop` (optional) completes with the batch's last kernel itself: an event bound to the
// dispatch (hipExtLaunchKernel) instead of a marker packet recorded after it (a barrier with an
// agent-scope release between two batches, ≈ 3.3 µs).
// (A timing pair armed by neb_time_next_kernel goes to the batch's first kernel: the main kernel, or
// the tail kernel of a small batch.)
extern "C" hipError_t neb_gcm_batch_single(int open, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                                           const uint32_t* d_keys, uint32_t max_keys, uint32_t key_hint,
                                           int32_t* d_status, const uint32_t* d_n, int cu_count, hipStream_t s,
                                           int hdr_from_dst, hipEvent_t stop, const uint8_t* rx) {
    neb::GcmArgs a{d_desc, n, d_arena, d_keys, max_keys, key_hint, d_status, d_n, (uint32_t)hdr_from_dst, 0u, rx};
    const uint32_t groups = (n + neb::kPpw - 1u) / neb::kPpw;
    const bool cs = !open && hdr_from_dst == 2;  // the TX seal with its checksums (tx.hip)
    if (!d_n && !cs && n <= neb::kSmallBatch) {
        a.tail_slots = neb::kTailAll;
        return launch_tail(open, rx, n, cu_count, s, stop, a);
    }
    const uint32_t slots = neb_gcm_single_slots(n, cu_count, open, hdr_from_dst);
    // a partial last pass (at most n packets; the real count may be on the device) goes to the
    // tail kernel, 64 lanes per packet
    const bool tail = groups > slots && (d_n || groups % slots);
    if (tail) a.tail_slots = slots;
    const dim3 grid(slots / neb::kSingleWaves);
    if (grid.x == 0) return hipSuccess;
    // the stop event goes to the batch's last kernel
    (void)neb::launch_bound(single_kernel_of(open, cs, rx), grid, dim3(neb::kSingleThreads), s, tail ? nullptr : stop, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !tail) return e;
    // the tail: exact for a host count; for a device count the largest one, under one pass and n
    // packets (a device count may leave a partial pass even when the bound n is a whole number of
    // passes)
    const uint32_t tail_pkts = d_n ? std::min(n, slots * neb::kPpw) : n - groups / slots * slots * neb::kPpw;
    return launch_tail(open, rx, tail_pkts, cu_count, s, stop, a);
}

// One packet (the per-packet path): aad[aad_len] and in[in_len] (payload, + tag when opening) go
// in the kernel arguments; the kernel writes len payload bytes (+ the tag when sealing) to `out`
// and the status to *status (pinned host memory, or device memory). hipErrorInvalidValue when the
// packet does not fit kOneBytes (the caller takes the batch path).
extern "C" hipError_t neb_gcm_one(int open, const uint8_t* aad, uint32_t aad_len, const uint8_t* in, uint32_t in_len,
                                  uint32_t len, uint64_t counter, uint8_t* out, int32_t* status, const uint32_t* d_keys,
                                  uint32_t max_keys, uint32_t key, hipStream_t s) {
    const uint32_t pay = (aad_len + 15u) & ~15u;
    if ((uint64_t)pay + in_len > neb::kOneBytes) return hipErrorInvalidValue;
    neb::OneArgs a;
    std::memset(&a, 0, offsetof(neb::OneArgs, in));
    if (aad_len) std::memcpy(a.in, aad, aad_len);
    if (in_len) std::memcpy(a.in + pay, in, in_len);
    a.d.aad_off = 0;
    a.d.src_off = pay;
    a.d.len = len;
    a.d.aad_len = aad_len;
    a.d.counter = counter;
    a.d.key_id = key;
    a.keys = d_keys;
    a.max_keys = max_keys;
    a.key = key;
    a.status = status;
    a.d.dst_off = (uint64_t)(uintptr_t)out;  // the output's address: the kernel rebases it on its argument block
    if (open)
        hipLaunchKernelGGL(neb::gcm_one_kernel<true>, dim3(1), dim3(neb::kOneFillThreads), 0, s, a);
    else
        hipLaunchKernelGGL(neb::gcm_one_kernel<false>, dim3(1), dim3(neb::kOneFillThreads), 0, s, a);
    return hipGetLastError();
}

// A combined launch of n per-packet requests (engine.cpp PktComb): descriptors, statuses and slots
// (kCombSlot bytes each, the descriptors' offsets from `slots`) in pinned host memory.
extern "C" hipError_t neb_gcm_one_batch(int open, const neb_desc* descs, int32_t* status, uint8_t* slots, uint32_t n,
                                        const uint32_t* d_keys, uint32_t max_keys, hipStream_t s) {
    if (n == 0 || n > neb::kCombMax) return hipErrorInvalidValue;
    neb::OneBatchDescs a;
    std::memcpy(a.d, descs, n * sizeof(neb_desc));
    const dim3 grid((n + neb::kOneBatchWaves - 1) / neb::kOneBatchWaves), block(neb::kOneBatchWaves * neb::kWave);
    if (open)
        hipLaunchKernelGGL(neb::gcm_one_batch_kernel<true>, grid, block, 0, s, a, status, slots, n, d_keys, max_keys);
    else
        hipLaunchKernelGGL(neb::gcm_one_batch_kernel<false>, grid, block, 0, s, a, status, slots, n, d_keys, max_keys);
    return hipGetLastError();
}

// Mixed keys: the batch has been regrouped into chunks by neb_sched_build.
extern "C" hipError_t neb_gcm_batch_chunked(int open, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                                            const uint32_t* d_keys, uint32_t max_keys, int32_t* d_status,
                                            const uint32_t* d_sorted, const uint4* d_chunks,
                                            uint32_t* d_counters, uint32_t max_chunks,
                                            int cu_count, hipStream_t s, int hdr_from_dst,
                                            hipEvent_t stop, const uint8_t* rx) {
    neb::GcmArgs a{d_desc, n, d_arena, d_keys, max_keys, NEB_KEYS_MIXED, d_status, nullptr, (uint32_t)hdr_from_dst, 0u, rx};
    neb::ChunkArgs ca{d_sorted, d_chunks, d_counters, max_chunks};
    // one workgroup per chunk up to the occupancy cap (tails make chunks outnumber n / 16), so a
    // small batch's chunks spread over the CUs; the chunk counts are only known on the device:
    // workgroups past them exit before filling their tables. Full chunks first, then the tails.
    const uint32_t bound = max_chunks * (uint32_t)neb::kChunkWaves;
    // stop (optional): an event bound to the kernel's dispatch (no marker packet after it)
    if (open && rx)
        return launch_grid_stop(neb::gcm_chunk_kernel<true, true>, neb::kChunkThreads, bound, cu_count, s, stop, a, ca);
    return open ? launch_grid_stop(neb::gcm_chunk_kernel<true>, neb::kChunkThreads, bound, cu_count, s, stop, a, ca)
                : launch_grid_stop(neb::gcm_chunk_kernel<false>, neb::kChunkThreads, bound, cu_count, s, stop, a, ca);
}

// ---- descriptor staging (not GCM: it lives here with the other batch launchers) ----------------

namespace neb {
// A host-staged chunk's descriptors from pinned host memory into device memory (engine.cpp
// batch_host), many loads in flight at once: the batch kernels then read them from HBM. Read in
// place, each wave's descriptor loads waited behind the staging copies' PCIe traffic.
__global__ __launch_bounds__(256) void copy_desc_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src,
                                                        uint32_t nvec) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nvec; i += gridDim.x * 256u) dst[i] = src[i];
}
}  // namespace neb

extern "C" hipError_t neb_copy_desc(neb_desc* dst, const neb_desc* src, uint32_t n, hipStream_t s) {
    static_assert(sizeof(neb_desc) % 16 == 0, "descriptors copy as 16-byte vectors");
    const uint32_t nvec = n * (uint32_t)(sizeof(neb_desc) / 16);
    if (!nvec) return hipSuccess;
    const uint32_t grid = std::min((nvec + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(neb::copy_desc_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<uint4*>(dst),
                       reinterpret_cast<const uint4*>(src), nvec);
    return hipGetLastError();
}

