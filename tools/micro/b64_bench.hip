// b64_bench.hip — the 5-bit GHASH window lookup against the nibble one (16 waves per CU):
//  B64:  ds_read_b64 at row*256 + (data & 31)*8: 32 entries × 8 B are one 256-byte row, so any 32
//        lanes read a row conflict-free whatever their entries (gf_mul_full5)
//  B128: ds_read_b128 at row*256 + (data & 15)*16, the nibble GHASH table's row pattern (gf_mul_full)
// Each lane runs CH independent chains of dependent lookups (the next entry comes from the data),
// so CH = 1 measures latency and CH = 8 throughput. Expected per wave instruction: 2 LDS cycles
// for B64, 4 for B128, no conflicts. With an argument (0..3) only that case runs, for a counter
// pass (SQ_LDS_IDX_ACTIVE, SQ_LDS_BANK_CONFLICT per wave instruction; the JSON line carries the
// wave-instruction count). Not part of the engine.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

constexpr int kThreads = 1024;
constexpr uint32_t kRows = 384;  // 96 KiB: one workgroup (16 waves) per CU

template <int WIDE, int CH>
__global__ __launch_bounds__(kThreads, 4) void k(uint32_t* out, int iters) {
    __shared__ uint4 tab[kRows * 16];  // row r at byte r*256
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kRows * 16u; i += kThreads) {
        const uint32_t h = i * 2654435761u;
        tab[i] = make_uint4(h, h ^ 0x9E3779B9u, h * 7u, h >> 3);
    }
    __syncthreads();
    uint32_t x[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) x[c] = tid * (2u * c + 1u);
    uint32_t row = 0;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const uint32_t base = (row + (uint32_t)c) << 8;  // row = step (row + c < kRows)
            const char* t = reinterpret_cast<const char*>(tab);
            if (WIDE) {
                const uint4 e = *reinterpret_cast<const uint4*>(__builtin_assume_aligned(t + (base | ((x[c] & 15u) << 4)), 16));
                x[c] ^= e.x ^ e.y ^ e.z ^ e.w;
            } else {
                const uint2 e = *reinterpret_cast<const uint2*>(__builtin_assume_aligned(t + (base | ((x[c] & 31u) << 3)), 8));
                x[c] ^= e.x ^ e.y;
            }
        }
        row = row + 8u < kRows - 8u ? row + 8u : 0u;
    }
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < CH; c++) r ^= x[c];
    out[blockIdx.x * kThreads + tid] = r;
}

template <int WIDE, int CH>
static void run(uint32_t* d_out, int blocks, int iters, int cus) {
    hipLaunchKernelGGL((k<WIDE, CH>), dim3(blocks), dim3(kThreads), 0, 0, d_out, iters);
    hipDeviceSynchronize();
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    float best = 1e30f;
    for (int r = 0; r < 5; r++) {
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL((k<WIDE, CH>), dim3(blocks), dim3(kThreads), 0, 0, d_out, iters);
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    const double wave_reads = (double)blocks * (kThreads / 64) * iters * CH;
    printf("{\"pattern\": \"%s\", \"chains\": %d, \"ms\": %.4f, \"wave_reads_per_launch\": %.0f, \"wave_reads_per_cu_per_ns\": %.4f}\n",
           WIDE ? "b128 nibble row" : "b64 5-bit row", CH, best, wave_reads, wave_reads / cus / (best * 1e6));
    fflush(stdout);
}

int main(int argc, char** argv) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) return 1;
    uint32_t* d_out;
    if (hipMalloc(&d_out, (size_t)cus * 4 * kThreads * 4) != hipSuccess) return 1;
    const int iters = 2000, only = argc > 1 ? atoi(argv[1]) : -1;
    if (only < 0 || only == 0) run<0, 1>(d_out, cus * 4, iters, cus);
    if (only < 0 || only == 1) run<1, 1>(d_out, cus * 4, iters, cus);
    if (only < 0 || only == 2) run<0, 8>(d_out, cus * 4, iters, cus);
    if (only < 0 || only == 3) run<1, 8>(d_out, cus * 4, iters, cus);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
