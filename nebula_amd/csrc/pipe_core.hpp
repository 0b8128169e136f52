// pipe_core.hpp — the pure parts of the staged host pipeline (engine.cpp batch_host): the chunk
// plan, a chunk's arena span with its descriptors rebased onto it, and the overlap test between
// the spans of chunks in flight. No HIP: tests/sanitize/pipe_test.cpp runs it on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/nebula_aead.h"

namespace neb {

// The staged host pipeline (batch_host, round 6): chunks of kPipeChunkPkts packets through
// kPipeSlots device buffers, with the copies in, the kernels and the copies back on three streams
// of their own, chained by events: chunk k + 1's copy-in then runs beside chunk k - 1's copy-back
// (PCIe carries both directions at once: 56 GB/s each alone, 96 GB/s together on this box).
// Chunks ramp up from kPipeFirst packets (doubling) to kPipeChunkPkts and back down at the end, so the
// first copy-in and the last copy-back, which run with nothing beside them, are short. A/B on C2
// (profiles/r6/host/): chunks of 4096 / 8192 / 12288 / 16384 / 32768 packets 23.9 / 26.6 / 32.6-33.2 /
// 32.6 / 28.5 GiB/s; a 16384-packet copy-in runs 395 µs alone and 520 µs beside a copy-back (42 + 51
// GB/s), and the first and last of each call ran alone for ≈ 0.9 of its 2.7 ms.
constexpr int kPipeSlots = 4;
#ifndef NEB_PIPE_CHUNK
#define NEB_PIPE_CHUNK 16384
#endif
#ifndef NEB_PIPE_FIRST
#define NEB_PIPE_FIRST 4096
#endif
constexpr uint32_t kPipeChunkPkts = NEB_PIPE_CHUNK;  // packets per staged host chunk at most
constexpr uint32_t kPipeFirst = NEB_PIPE_FIRST;      // the first and last chunks' packets

// chunk sizes for a batch of n packets: kPipeFirst, 2 kPipeFirst, ... up to kPipeChunkPkts at both
// ends (while the rest still holds 4x the next size), full chunks between
inline std::vector<uint32_t> pipe_plan(uint32_t n) {
    std::vector<uint32_t> head, plan;
    uint32_t rem = n;
    for (uint32_t s = kPipeFirst; s < kPipeChunkPkts && rem >= 4u * s; s *= 2u) {
        head.push_back(s);
        rem -= 2u * s;
    }
    plan = head;
    for (; rem; rem -= std::min(rem, kPipeChunkPkts)) plan.push_back(std::min(rem, kPipeChunkPkts));
    plan.insert(plan.end(), head.rbegin(), head.rend());
    return plan;
}

// The bytes [lo, hi) of the arena that a chunk copies in and back.
struct PipeSpan {
    uint64_t lo = 0, hi = 0;
    // A chunk copies its whole span back, so the spans of two chunks in flight must not share a byte.
    bool overlaps(const PipeSpan& o) const { return lo < o.hi && o.lo < hi; }
};

// The span of cnt > 0 descriptors that lie inside the arena (neb_desc_in_arena, so no sum below
// wraps): from the lowest byte any of them reads or writes, rounded down to 16 so that the device
// buffer holds the arena at the same alignment modulo 16, to the highest.
inline PipeSpan pipe_span(const neb_desc* desc, uint32_t cnt, int open) {
    uint64_t lo = ~0ULL, hi = 0;
    for (uint32_t i = 0; i < cnt; i++) {
        const neb_desc& d = desc[i];
        const uint64_t pay = (uint64_t)d.len + (open ? 16u : 0u), outl = (uint64_t)d.len + (open ? 0u : 16u);
        lo = std::min({lo, d.src_off, d.dst_off, d.aad_off});
        hi = std::max({hi, d.src_off + pay, d.dst_off + outl, d.aad_off + d.aad_len});
    }
    return {lo & ~(uint64_t)15, hi};
}

// The chunk's descriptors as offsets into its device buffer, which holds the arena from lo.
inline void pipe_rebase(neb_desc* out, const neb_desc* desc, uint32_t cnt, uint64_t lo) {
    for (uint32_t i = 0; i < cnt; i++) {
        neb_desc d = desc[i];
        d.src_off -= lo;
        d.aad_off -= lo;
        d.dst_off -= lo;
        out[i] = d;
    }
}

}  // namespace neb
