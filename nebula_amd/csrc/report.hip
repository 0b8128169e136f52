// report.hip — the RX batch report on the device: a finished receive batch's statuses, headers,
// tunnels and sources -> runs per (tunnel, source), relay indexes used, the host's work list and the
// metric counts. Rules: report_core.hpp.
//
// The host form walks the packets once and sorts the authenticated ones. Here:
//   classify   one thread per packet: the header and status rules, the metrics (summed per workgroup
//              in LDS, then one set of atomics per workgroup), the work kind, and two 33-bit sort keys
//   sort       the packets by tunnel key (stable, so by (key_id, packet index)) and the relay keys;
//              packets that are in neither carry the key 2^32 and end up behind the others
//   heads      one thread per sorted position: run, tunnel and relay-index heads, the wire length
//   scan       three exclusive sums over n + 1 elements; element n holds the totals
//   place      work records, and where every run and every relay index starts; the counts
//   emit       one thread per run and per relay index: a segment is [start[r], start[r + 1]), its
//              packets the difference of the positions, its bytes the difference of the length sums
// Grid-wide dependencies are separate launches; nothing spins.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "../../include/nebula_aead.h"
#include "report.hpp"
#include "report_core.hpp"

namespace neb {

constexpr uint32_t kReportThreads = 256;
constexpr uint32_t kReportSlots = NEB_METRIC_NO_TUNNEL + 1u;  // the slots that are counted

// The ABI aligns the packet records to 4 bytes.
__device__ inline neb_rx_packet report_get_pk(const neb_rx_packet* pk, uint32_t i) {
    const uint32_t* p = static_cast<const uint32_t*>(__builtin_assume_aligned(&pk[i], 4));
    return neb_rx_packet{(uint64_t)p[0] | (uint64_t)p[1] << 32, p[2], p[3]};
}
__device__ inline void report_put2(void* dst, uint32_t a, uint32_t b) {
    uint32_t* p = static_cast<uint32_t*>(__builtin_assume_aligned(dst, 4));
    p[0] = a, p[1] = b;
}

__global__ void __launch_bounds__(kReportThreads) report_classify_kernel(ReportArgs a) {
    __shared__ unsigned long long sm[kReportSlots];
    const uint32_t i = blockIdx.x * kReportThreads + threadIdx.x;
    if (threadIdx.x < kReportSlots) sm[threadIdx.x] = 0ull;
    __syncthreads();
    if (i < a.n) {
        const neb_rx_packet p = report_get_pk(a.pk, i);
        uint8_t h[16] = {};
        if ((p.len & ~NEB_RX_OWN_SOURCE) >= 16u) {
            const uint8_t* src = a.arena + p.off;
            h[0] = src[0], h[1] = src[1];
            for (int k = 4; k < 8; k++) h[k] = src[k];
        }
        const ReportPacket r = report_packet(a.status[i], p.len, p.key_id, h, a.relayed != 0u);
        if (r.invalid) atomicAdd(&sm[NEB_METRIC_RX_INVALID], 1ull);
        if (r.rx_slot != kReportNoSlot) atomicAdd(&sm[r.rx_slot], 1ull);
        if (r.status_slot != kReportNoSlot) atomicAdd(&sm[r.status_slot], 1ull);
        if (r.auth) atomicAdd(&sm[NEB_METRIC_OPENED_BYTES], (unsigned long long)r.len);
        a.ws.work[i] = r.work;
        a.ws.tun_key[i] = r.auth ? (uint64_t)p.key_id : kReportNoKey;
        a.ws.tun_idx[i] = i;
        a.ws.relay_key[i] = r.relay ? (uint64_t)r.relay_index : kReportNoKey;
    }
    __syncthreads();
    if (threadIdx.x < kReportSlots && sm[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(&a.metrics[threadIdx.x]), sm[threadIdx.x]);
}

__global__ void __launch_bounds__(kReportThreads) report_heads_kernel(ReportArgs a) {
    const uint32_t j = blockIdx.x * kReportThreads + threadIdx.x;
    if (j > a.n) return;
    uint64_t work = 0, run = 0, tun = 0, relay = 0, len = 0;
    if (j < a.n) {
        work = a.ws.work[j] != 0u;
        const uint64_t k = a.ws.tun_key_s[j];
        if (k < kReportNoKey) {  // authenticated; so is every position before it
            const uint32_t i = a.ws.tun_idx_s[j];
            len = report_get_pk(a.pk, i).len & ~NEB_RX_OWN_SOURCE;
            tun = j == 0u || a.ws.tun_key_s[j - 1u] != k;
            run = tun || !report_same_from(report_from(a.from, a.pkt_entry, a.nfrom, i, a.relayed != 0u),
                                           report_from(a.from, a.pkt_entry, a.nfrom, a.ws.tun_idx_s[j - 1u], a.relayed != 0u));
            if (j + 1u == a.n || a.ws.tun_key_s[j + 1u] >= kReportNoKey) a.ws.ends[0] = j + 1u;
        }
        const uint64_t rk = a.ws.relay_key_s[j];
        if (rk < kReportNoKey) {
            relay = j == 0u || a.ws.relay_key_s[j - 1u] != rk;
            if (j + 1u == a.n || a.ws.relay_key_s[j + 1u] >= kReportNoKey) a.ws.ends[1] = j + 1u;
        }
    }
    a.ws.flag_a[j] = work | run << 32;
    a.ws.flag_b[j] = tun | relay << 32;
    a.ws.len[j] = len;
}

__global__ void __launch_bounds__(kReportThreads) report_place_kernel(ReportArgs a) {
    const uint32_t j = blockIdx.x * kReportThreads + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t fa = a.ws.flag_a[j], fb = a.ws.flag_b[j], sa = a.ws.sum_a[j], sb = a.ws.sum_b[j];
    if ((uint32_t)fa) report_put2(&a.work[(uint32_t)sa], j, a.ws.work[j]);
    if (fa >> 32) a.ws.run_start[(uint32_t)(sa >> 32)] = j;
    if (fb >> 32) a.ws.relay_start[(uint32_t)(sb >> 32)] = j;
    if (j == 0u) {
        const uint64_t ta = a.ws.sum_a[a.n], tb = a.ws.sum_b[a.n];
        a.counts[0] = (uint32_t)(ta >> 32);  // nruns
        a.counts[1] = (uint32_t)tb;          // ntunnels
        a.counts[2] = (uint32_t)(tb >> 32);  // nrelay_used
        a.counts[3] = (uint32_t)ta;          // nwork
    }
}

__global__ void __launch_bounds__(kReportThreads) report_emit_kernel(ReportArgs a) {
    const uint32_t r = blockIdx.x * kReportThreads + threadIdx.x;
    if (r >= a.n) return;
    const uint32_t nruns = (uint32_t)(a.ws.sum_a[a.n] >> 32), nrelay = (uint32_t)(a.ws.sum_b[a.n] >> 32);
    if (r < nruns) {
        const uint32_t s = a.ws.run_start[r], e = r + 1u < nruns ? a.ws.run_start[r + 1u] : a.ws.ends[0];
        const uint32_t i = a.ws.tun_idx_s[s];
        report_put_run(&a.runs[r], a.ws.sum_len[e] - a.ws.sum_len[s], (uint32_t)a.ws.tun_key_s[s], i, e - s,
                       report_from(a.from, a.pkt_entry, a.nfrom, i, a.relayed != 0u));
    }
    if (r < nrelay) {
        const uint32_t s = a.ws.relay_start[r], e = r + 1u < nrelay ? a.ws.relay_start[r + 1u] : a.ws.ends[1];
        report_put2(&a.relay_used[r], (uint32_t)a.ws.relay_key_s[s], e - s);
    }
}

}  // namespace neb

extern "C" size_t neb_report_ws_bytes(uint32_t n, size_t* cub_bytes) {
    using namespace neb;
    size_t pairs = 0, keys = 0, scan = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, pairs, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                       (uint32_t*)nullptr, n, 0, kReportKeyBits);
    hipcub::DeviceRadixSort::SortKeys(nullptr, keys, (const uint64_t*)nullptr, (uint64_t*)nullptr, n, 0, kReportKeyBits);
    hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (const uint64_t*)nullptr, (uint64_t*)nullptr, n + 1u);
    *cub_bytes = std::max({pairs, keys, scan, (size_t)256});
    return report_ws_layout(n, *cub_bytes, nullptr, nullptr);
}

extern "C" hipError_t neb_report_run(const neb::ReportArgs* args, hipStream_t s) {
    using namespace neb;
    const ReportArgs& a = *args;
    const ReportWs& w = a.ws;
    const dim3 tpb(kReportThreads);
    const dim3 grid((a.n + kReportThreads - 1) / kReportThreads), grid1(a.n / kReportThreads + 1u);  // n, n + 1 threads
    size_t cub = 0;
    if (neb_report_ws_bytes(a.n, &cub), cub > w.cub_bytes) return hipErrorInvalidValue;  // laid out for fewer packets
    hipError_t e = hipMemsetAsync(a.metrics, 0, kReportMetrics * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(report_classify_kernel, grid, tpb, 0, s, a);
    size_t cb = w.cub_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(w.cub_tmp, cb, w.tun_key, w.tun_key_s, w.tun_idx, w.tun_idx_s, a.n, 0,
                                           kReportKeyBits, s);
    if (e != hipSuccess) return e;
    cb = w.cub_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(w.cub_tmp, cb, w.relay_key, w.relay_key_s, a.n, 0, kReportKeyBits, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(report_heads_kernel, grid1, tpb, 0, s, a);
    const uint64_t* in[3] = {w.flag_a, w.flag_b, w.len};
    uint64_t* out[3] = {w.sum_a, w.sum_b, w.sum_len};
    for (int k = 0; k < 3; k++) {
        cb = w.cub_bytes;
        e = hipcub::DeviceScan::ExclusiveSum(w.cub_tmp, cb, in[k], out[k], a.n + 1u, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(report_place_kernel, grid, tpb, 0, s, a);
    hipLaunchKernelGGL(report_emit_kernel, grid, tpb, 0, s, a);
    return hipGetLastError();
}
