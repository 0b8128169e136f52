// recv.hip — the RX receive plan on the device: recvmmsg entries with UDP_GRO -> wire packets,
// ListenOut's getFrom / parseRecvCmsg / deliverSegments for a whole batch.
//
// The reference walks entry after entry; where one entry's packets end decides where the next one's
// start. Here (rules: recv_core.hpp):
//   entry   one thread per entry: the cmsg walk (or the caller's size), its packet count, from[]
//   scan    exclusive sum of the counts in 64 bits: first[]
//   emit    one thread per output slot: the entry whose packets hold the slot, then its records; and
//           one thread per entry: entry_first[], and the counts where the emitted prefix ends
// The work of emit follows the output slots, not the entries: one entry may hold 65 535 packets
// beside thousands that hold one. Each slot finds its entry by a binary search over first[], at most
// 31 dependent loads that stay in L2 (measured against one search per workgroup and a narrowed
// search per thread, which lost on every shape: DESIGN.md §3.16).
// Grid-wide dependencies are separate launches; nothing spins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <hipcub/hipcub.hpp>

#include "../../include/nebula_aead.h"
#include "recv.hpp"
#include "recv_core.hpp"

namespace neb {

constexpr uint32_t kRecvThreads = 256;

// The ABI aligns the per-packet and per-entry outputs to 4 bytes: records go out as words.
__device__ inline void recv_put5(void* dst, const RecvFrom& f, uint32_t last) {
    uint32_t* p = static_cast<uint32_t*>(__builtin_assume_aligned(dst, 4));
    p[0] = f.a[0], p[1] = f.a[1], p[2] = f.a[2], p[3] = f.a[3], p[4] = last;
}
__device__ inline void recv_put_pk(neb_rx_packet* dst, uint64_t off, uint32_t len) {
    uint32_t* p = static_cast<uint32_t*>(__builtin_assume_aligned(dst, 4));
    p[0] = (uint32_t)off, p[1] = (uint32_t)(off >> 32), p[2] = len, p[3] = NEB_KEYS_MIXED;
}
__device__ inline RecvFrom recv_entry_from(const neb_recv_entry* en, uint32_t socket_v4) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(en) + 4;  // name, at byte 16
    const uint32_t name[7] = {w[0], w[1], w[2], w[3], w[4], w[5], w[6]};
    return recv_from(name, socket_v4);
}

__global__ void __launch_bounds__(kRecvThreads) recv_entry_kernel(RecvArgs a) {
    const uint32_t j = blockIdx.x * kRecvThreads + threadIdx.x;
    if (j >= a.n) return;
    const neb_recv_entry* en = &a.entries[j];
    const int32_t seg = recv_seg_size(*en, a.ctrl, a.ctrl_stride, j);
    a.ws.seg[j] = seg;
    a.ws.cnt[j] = recv_count(en->len, seg);
    if (a.from) {
        const RecvFrom f = recv_entry_from(en, a.socket_v4);
        recv_put5(&a.from[j], f, recv_addr_word(f));
    }
}

// The largest j in [lo, hi] with first[j] <= i; first[lo] <= i.
__device__ inline uint32_t recv_find(const uint64_t* first, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (first[mid] <= i) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

__global__ void __launch_bounds__(kRecvThreads) recv_emit_kernel(RecvArgs a) {
    const uint32_t t = blockIdx.x * kRecvThreads + threadIdx.x;
    // per entry: entry_first[], and the counts at the end of the emitted prefix
    if (t < a.n) {
        const uint64_t f = a.ws.first[t], c = a.ws.cnt[t];
        const bool em = recv_emitted(f, c, a.max_packets);
        a.entry_first[t] = em ? (uint32_t)f : NEB_RECV_NONE;
        if (em && (t + 1u == a.n || !recv_emitted(f + c, a.ws.cnt[t + 1u], a.max_packets))) {
            a.counts[0] = (uint32_t)(f + c);
            a.counts[1] = t + 1u;
        }
        if (t == 0u && !em) a.counts[0] = a.counts[1] = 0u;
    } else if (t == 0u) {
        a.counts[0] = a.counts[1] = 0u;
    }
    // per output slot
    if (t >= a.max_packets) return;
    bool pad = true;
    if (a.n) {
        const uint32_t j = recv_find(a.ws.first, 0, a.n - 1u, t);
        const uint64_t f = a.ws.first[j], c = a.ws.cnt[j], k = t - f;
        if (recv_emitted(f, c, a.max_packets) && k < c) {
            pad = false;
            const neb_recv_entry* en = &a.entries[j];
            uint64_t off;
            uint32_t len;
            recv_packet(en->off, en->len, a.ws.seg[j], k, &off, &len);
            recv_put_pk(&a.pk[t], off, len);
            if (a.pkt_entry) a.pkt_entry[t] = j;
            if (a.src) {
                const RecvFrom fr = recv_entry_from(en, a.socket_v4);
                recv_put5(&a.src[t], fr, recv_source_word(fr));
            }
        }
    }
    if (pad) {  // the receive calls' gate refuses it
        recv_put_pk(&a.pk[t], 0, 0);
        if (a.pkt_entry) a.pkt_entry[t] = NEB_RECV_NONE;
        if (a.src) recv_put5(&a.src[t], RecvFrom{}, 0u);
    }
}

}  // namespace neb

extern "C" size_t neb_recv_ws_bytes(uint32_t n, size_t* cub_bytes) {
    using namespace neb;
    size_t c = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, c, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n);
    *cub_bytes = c;
    return recv_ws_layout(n, c, nullptr, nullptr);
}

extern "C" hipError_t neb_recv_run(const neb::RecvArgs* args, hipStream_t s) {
    using namespace neb;
    const RecvArgs& a = *args;
    const dim3 tpb(kRecvThreads);
    if (a.n) {
        hipLaunchKernelGGL(recv_entry_kernel, dim3((a.n + kRecvThreads - 1) / kRecvThreads), tpb, 0, s, a);
        size_t cb = a.ws.cub_bytes;
        hipError_t e = hipcub::DeviceScan::ExclusiveSum(a.ws.cub_tmp, cb, a.ws.cnt, a.ws.first, (int)a.n, s);
        if (e != hipSuccess) return e;
    }
    const uint32_t threads = std::max({a.n, a.max_packets, 1u});
    hipLaunchKernelGGL(recv_emit_kernel, dim3((threads + kRecvThreads - 1) / kRecvThreads), tpb, 0, s, a);
    return hipGetLastError();
}
