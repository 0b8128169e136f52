// gcm_trace.hpp — the build-time instrumentation of the GCM kernels (aes_gcm.hip), all of it here:
//   -DNEB_ISA_MARKS     NEB_MARK(x): region markers in the kernels' assembly
//   -DNEB_WAVE_TRACE=1  the wave timeline and per-wave phase times of the single-key and chunk
//                       kernels, fetched by tools/wave_trace.py through neb_debug_wave_trace
//   -DNEB_ONE_TRACE=1   phase stamps of the per-packet kernel, printed by lane 0 (tools/one_trace.py)
// The kernels and gcm_packet_group call GroupTrace, WaveTimeline and OneTrace unconditionally; in the
// product build these are empty types, and it has none of the instrumentation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/nebula_aead.h"

#ifdef NEB_ISA_MARKS
#define NEB_MARK(x) asm volatile(";NEBMARK " #x)
#else
#define NEB_MARK(x) ((void)0)
#endif

namespace neb {

#ifdef NEB_WAVE_TRACE
// Timeline records, in s_memrealtime ticks (100 MHz): per chunk {workgroup << 20 | wave << 16 |
// count << 8 | lg << 4 | full, chunk index, start, end}, and per wave {…, ~0u, kernel start, tables
// filled}. Fixed slots per wave (no shared counter: one atomic word serialised the waves and skewed
// the timeline it was meant to record): slot 0 the wave's start, slot 1 + k its k-th chunk.
constexpr uint32_t kWaveTraceSlots = 64, kWaveTraceWaves = 8192, kWaveTraceCap = kWaveTraceSlots * kWaveTraceWaves;
__device__ uint4 g_wtrace[kWaveTraceCap];
// Per-wave phase times of the packet groups: the chunk kernel clears them per chunk and records
// them; ticks summed over the chunk's groups, each phase closed by a full s_waitcnt (so a phase's
// time includes the latency of its own accesses)
constexpr uint32_t kWavePhaseWaves = 8192;
__device__ uint32_t g_wphase[kWavePhaseWaves * 4];  // desc, rounds, final, finish
__device__ __forceinline__ uint32_t wave_gid() { return blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
__device__ __forceinline__ void wave_trace(uint32_t lane, uint32_t slot, uint32_t a, uint32_t b, uint64_t t0,
                                           uint64_t t1) {
    const uint32_t w = wave_gid();
    if (lane == 0u && w < kWaveTraceWaves && slot < kWaveTraceSlots)
        g_wtrace[w * kWaveTraceSlots + slot] = make_uint4(a | 0x80000000u, b, (uint32_t)t0, (uint32_t)t1);
}
__device__ __forceinline__ uint64_t phase_now() {
    __builtin_amdgcn_s_waitcnt(0);
    return __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void phase_add(uint32_t k, uint64_t t0, uint64_t t1) {
    const uint32_t w = wave_gid();
    if ((threadIdx.x & 63u) == 0u && w < kWavePhaseWaves) g_wphase[4u * w + k] += (uint32_t)(t1 - t0);
}

// A packet group's phases: close(k) adds the time since begin() or the last close() to phase k.
struct GroupPhases {
    uint64_t t;
    __device__ __forceinline__ void begin() { t = phase_now(); }
    __device__ __forceinline__ void close(uint32_t k) {
        const uint64_t t1 = phase_now();
        phase_add(k, t, t1);
        t = t1;
    }
};

// A wave's timeline in the single-key and chunk kernels.
struct WaveTimeline {
    uint32_t tag, k;
    uint64_t tk0, tc0, tcd, tck, tcs;
    __device__ __forceinline__ void kernel_begin(uint32_t wave) {
        tag = blockIdx.x << 20 | wave << 16;
        tk0 = __builtin_amdgcn_s_memrealtime();
    }
    __device__ __forceinline__ void tables_filled(uint32_t lane) {
        k = 1;
        wave_trace(lane, 0, tag, ~0u, tk0, __builtin_amdgcn_s_memrealtime());
    }
    __device__ __forceinline__ void chunk_begin() { tc0 = __builtin_amdgcn_s_memrealtime(); }
    // shape: count << 8 | lg << 4 | full
    __device__ __forceinline__ void chunk_end(uint32_t lane, uint32_t shape, uint32_t index) {
        wave_trace(lane, k++, tag | shape, index, tc0, __builtin_amdgcn_s_memrealtime());
    }
    // The chunk kernel's phases: {descriptor in, round keys in, tables staged} and the groups' sums
    __device__ __forceinline__ void phases_begin(uint32_t lane) {
        if (lane == 0u && wave_gid() < kWavePhaseWaves)
            for (uint32_t i = 0; i < 4u; i++) g_wphase[4u * wave_gid() + i] = 0u;
        tcd = phase_now();
    }
    __device__ __forceinline__ void keys_in() { tcs = tck = phase_now(); }
    __device__ __forceinline__ void tables_staged() { tcs = phase_now(); }
    __device__ __forceinline__ void phases_end(uint32_t lane) {  // (after chunk_end)
        if (k > 21u) return;
        const uint32_t w = wave_gid() < kWavePhaseWaves ? wave_gid() : 0u;
        const uint32_t* ph = &g_wphase[4u * w];
        wave_trace(lane, 20u + 2u * (k - 1u), tag, 0xFFFFFFFEu, (uint32_t)(tcd - tc0) | (uint32_t)(tck - tcd) << 16,
                   (uint32_t)(tcs - tck));
        wave_trace(lane, 21u + 2u * (k - 1u), tag, 0xFFFFFFFDu, ph[0] | ph[1] << 16, ph[2] | ph[3] << 16);
    }
};
#else
struct GroupPhases {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void close(uint32_t) {}
};
struct WaveTimeline {
    __device__ __forceinline__ void kernel_begin(uint32_t) {}
    __device__ __forceinline__ void tables_filled(uint32_t) {}
    __device__ __forceinline__ void chunk_begin() {}
    __device__ __forceinline__ void chunk_end(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void phases_begin(uint32_t) {}
    __device__ __forceinline__ void keys_in() {}
    __device__ __forceinline__ void tables_staged() {}
    __device__ __forceinline__ void phases_end(uint32_t) {}
};
#endif

#if NEB_ONE_TRACE
// Stamps (100 MHz) printed by lane 0: an A/B build only. GroupStamps: a packet group's rounds and
// final; OneTrace: gcm_one_kernel's fill, round keys and packet.
struct GroupStamps {
    uint64_t t0, t1;
    __device__ __forceinline__ void rounds_begin() { t0 = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void rounds_done() {
        __builtin_amdgcn_s_waitcnt(0);
        t1 = __builtin_amdgcn_s_memrealtime();
    }
    __device__ __forceinline__ void final_done(uint32_t lane, uint32_t R) {
        __builtin_amdgcn_s_waitcnt(0);
        const uint64_t t2 = __builtin_amdgcn_s_memrealtime();
        if (lane == 0) printf("  rounds %u  final %u (x10 ns, R=%u)\n", (unsigned)(t1 - t0), (unsigned)(t2 - t1), R);
    }
};
struct OneTrace {
    uint64_t t0, t1, t2;
    __device__ __forceinline__ void kernel_begin() { t0 = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void filled() { t1 = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void keyed() { t2 = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ void done(uint32_t lane, bool open) {
        __builtin_amdgcn_s_waitcnt(0);
        const uint64_t t3 = __builtin_amdgcn_s_memrealtime();
        if (lane == 0)
            printf("one %d: fill %u  keys %u  packet %u  (x10 ns)\n", (int)open, (unsigned)(t1 - t0), (unsigned)(t2 - t1),
                   (unsigned)(t3 - t2));
    }
};
#else
struct GroupStamps {
    __device__ __forceinline__ void rounds_begin() {}
    __device__ __forceinline__ void rounds_done() {}
    __device__ __forceinline__ void final_done(uint32_t, uint32_t) {}
};
struct OneTrace {
    __device__ __forceinline__ void kernel_begin() {}
    __device__ __forceinline__ void filled() {}
    __device__ __forceinline__ void keyed() {}
    __device__ __forceinline__ void done(uint32_t, bool) {}
};
#endif

// What gcm_packet_group records: the wave-trace phases (descriptor, rounds, final, finish) and the
// per-packet build's stamps.
struct GroupTrace {
    GroupPhases ph;
    GroupStamps st;
    __device__ __forceinline__ void begin() { ph.begin(); }
    __device__ __forceinline__ void desc_in() { ph.close(0); }
    __device__ __forceinline__ void rounds_begin() { st.rounds_begin(); }
    __device__ __forceinline__ void rounds_done() {
        st.rounds_done();
        ph.close(1);
    }
    __device__ __forceinline__ void final_done(uint32_t lane, uint32_t R) {
        ph.close(2);
        st.final_done(lane, R);
    }
    __device__ __forceinline__ void finished() { ph.close(3); }
};

}  // namespace neb

#ifdef NEB_WAVE_TRACE
// tools/wave_trace.py: copy out (at most max entries) and reset the wave timeline
extern "C" NEB_API int neb_debug_wave_trace(void* out, uint32_t max) {
    void* d = nullptr;
    if (hipDeviceSynchronize() != hipSuccess || hipGetSymbolAddress(&d, HIP_SYMBOL(neb::g_wtrace)) != hipSuccess)
        return -1;
    const uint32_t n = std::min(neb::kWaveTraceCap, max);
    if (hipMemcpy(out, d, (size_t)n * 16u, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemset(d, 0, (size_t)neb::kWaveTraceCap * 16u) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return -1;
    return (int)n;
}
#endif
