// relay.hip — the forward half of a relay node's receive batch on the device
// (neb_relay_forward_batch, window.cpp): handleOutsideRelayPacket's ForwardingType branch
// (outside.go:220-240) and SendVia (inside.go:442-501) for every verified Message/Relay packet of
// the batch, with the counters SendVia would have taken packet by packet. On the stream, after the
// receive has written its statuses:
//
//   mark      one thread per packet (neb_relay_gate): its target tunnel when it takes a counter,
//             else its final fwd_status (NOT_FORWARDED / BAD_KEY).
//   rank      a stable sort by tunnel keeps arrival order inside each tunnel's run; a packet's
//             counter is its tunnel's message counter + its place in the run (counters follow
//             arrival order per tunnel, as NextMessageCounter hands them out).
//   send via  per packet (neb_relay_send_via): EXHAUSTED, or the new header over the old one and
//             the AD-only seal descriptor, compacted so the seal never sees another packet.
//   counters  each tunnel's message counter advances by its run, after every read of the old value.
//
// Two forms, as the TX plan (tx.hip): up to kRelayPlanSmallMax packets one workgroup does all of it
// in one launch (block radix sort + block scans; past one packet per thread the mark runs grid-wide
// first: it is a chain of dependent loads per packet); above that, the device-wide sort and
// scan-by-key. The existing seal then runs on the compacted batch, and neb_relay_fix copies back
// the rare seal status that is not OK.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "../../include/nebula_aead.h"
#include "device_common.hpp"
#include "layout.hpp"
#include "relay.hpp"

namespace neb {

struct RelayArgs {
    const neb_rx_packet* pk;
    const neb_relay_route* route;
    const int32_t* status;
    uint32_t n;
    neb_tx_tunnel* tun;
    uint32_t ntun;
    const uint32_t* keys;
    uint32_t max_keys;
    int alg;
    uint8_t* arena;
    int32_t* fwd_status;
    RelayWs ws;
};

// Packet i's sort key: its target tunnel when it takes a counter, else ntun (and its fwd_status).
__device__ __forceinline__ uint32_t relay_mark_one(const RelayArgs& a, uint32_t i) {
    const int32_t st = a.status[i];
    const neb_relay_route r = a.route[i];
    uint8_t h[2] = {0, 0};
    if (st == NEB_STATUS_OK && r.tunnel != NEB_RELAY_NONE) {
        const uint8_t* p = a.arena + a.pk[i].off;
        h[0] = p[0];
        h[1] = p[1];
    }
    const int32_t g = neb_relay_gate(st, h, r, a.tun, a.ntun, [&](uint32_t key) {
        return key < a.max_keys && a.keys[(size_t)key * kKeyRecDwords + kRecAlg] == (uint32_t)a.alg;
    });
    if (g != NEB_STATUS_OK) a.fwd_status[i] = g;
    return g == NEB_STATUS_OK ? r.tunnel : a.ntun;
}

// Packet i took counter c of tunnel t: its fwd_status; forwarded: the header and the seal
// descriptor at compacted position j. Returns whether it is forwarded.
__device__ __forceinline__ bool relay_exhausted(uint64_t c) { return c >= kRejectAfterMessages; }
__device__ __forceinline__ void relay_send_one(const RelayArgs& a, uint32_t i, uint32_t t, uint64_t c, uint32_t j) {
    const neb_rx_packet p = a.pk[i];
    uint32_t hdr[4];
    neb_desc d;
    const int32_t st = neb_relay_send_via(p, a.route[i].remote_index, a.tun[t].key_id, c, hdr, &d);
    a.fwd_status[i] = st;
    if (st != NEB_STATUS_OK) return;
    store_block(a.arena + p.off, make_uint4(hdr[0], hdr[1], hdr[2], hdr[3]), 16u);  // any byte address
    a.ws.sub_desc[j] = d;
    a.ws.sub_map[j] = i;
}

__global__ __launch_bounds__(256) void relay_mark_kernel(RelayArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) *a.ws.nsub = 0;
    if (i >= a.n) return;
    a.ws.key[i] = relay_mark_one(a, i);
    a.ws.idx[i] = i;
}

// ---- the whole plan in one workgroup (n <= kRelayPlanSmallMax) --------------------------------
//
// Thread t owns packets IT*t .. IT*t+IT-1 (blocked, arrival order), so the stable block sort by
// tunnel leaves every tunnel's run in arrival order; sorted position r of a run whose head is at
// position h has rank r - h + 1 (h by a block-wide running maximum of the head positions).
template <uint32_t IT, bool MARKED>
__global__ __launch_bounds__(kRelayPlanThreads) void relay_plan_small_kernel(RelayArgs a, int key_bits) {
    static_assert(IT <= kRelayPlanItems, "the LDS array holds kRelayPlanSmallMax packets");
    using Sort = hipcub::BlockRadixSort<uint32_t, kRelayPlanThreads, IT, uint32_t>;
    using Scan = hipcub::BlockScan<uint32_t, kRelayPlanThreads>;
    __shared__ union {
        typename Sort::TempStorage sort;
        typename Scan::TempStorage scan;
    } tmp;
    __shared__ uint32_t s_key[kRelayPlanThreads * IT];

    const uint32_t t = threadIdx.x, n = a.n, ntun = a.ntun;
    // 1. mark, packets striped over the threads; then each thread takes its blocked IT
    for (uint32_t i = t; i < kRelayPlanThreads * IT; i += kRelayPlanThreads)
        s_key[i] = i >= n ? ntun : MARKED ? a.ws.key[i] : relay_mark_one(a, i);
    __syncthreads();
    uint32_t key[IT], idx[IT];
#pragma unroll
    for (uint32_t k = 0; k < IT; k++) {
        idx[k] = t * IT + k;
        key[k] = s_key[idx[k]];
    }
    __syncthreads();
    // 2. ranks: a stable sort by tunnel, then each run's head position
    Sort(tmp.sort).Sort(key, idx, 0, key_bits);
#pragma unroll
    for (uint32_t k = 0; k < IT; k++) s_key[t * IT + k] = key[k];
    __syncthreads();
    uint32_t head[IT], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < IT; k++) {
        const uint32_t r = t * IT + k;
        head[k] = (r == 0u || s_key[r - 1u] != key[k]) ? r : 0u;
        mine = max(mine, head[k]);
    }
    uint32_t run;
    Scan(tmp.scan).ExclusiveScan(mine, run, 0u, hipcub::Max());
    // 3. counters; which packets are forwarded
    uint64_t ctr[IT];
    uint32_t nfwd = 0;
#pragma unroll
    for (uint32_t k = 0; k < IT; k++) {
        const uint32_t r = t * IT + k;
        run = max(run, head[k]);
        ctr[k] = 0;
        if (key[k] < ntun) {
            ctr[k] = a.tun[key[k]].message_counter + (r - run + 1u);
            nfwd += !relay_exhausted(ctr[k]);
        }
    }
    __syncthreads();  // tmp is reused; every read of the old counters is done
    uint32_t j, total;
    Scan(tmp.scan).ExclusiveSum(nfwd, j, total);
    // 4. send via; the last packet of a tunnel's run leaves the tunnel's new counter
#pragma unroll
    for (uint32_t k = 0; k < IT; k++) {
        const uint32_t r = t * IT + k;
        if (key[k] < ntun) {
            relay_send_one(a, idx[k], key[k], ctr[k], j);
            j += !relay_exhausted(ctr[k]);
            if (r + 1u == kRelayPlanThreads * IT || s_key[r + 1u] != key[k]) a.tun[key[k]].message_counter = ctr[k];
        }
    }
    if (t == 0) *a.ws.nsub = total;
}

// ---- the grid-wide form ----------------------------------------------------------------------

// One thread per sorted position. Forwarded packets take their compacted positions from one atomic
// per wave (the seal's results do not depend on the order of its batch).
__global__ __launch_bounds__(256) void relay_scatter_kernel(RelayArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t t = r < a.n ? a.ws.key_sorted[r] : a.ntun;
    const bool counted = t < a.ntun;
    uint64_t c = 0;
    uint32_t i = 0;
    if (counted) {
        i = a.ws.idx_sorted[r];
        const uint32_t rank = a.ws.rank[r];
        // relay_finish_kernel advances the counters only after this kernel has run
        c = a.tun[t].message_counter + rank + 1u;
        if (r + 1u == a.n || a.ws.key_sorted[r + 1u] != t) a.ws.tun_total[t] = rank + 1u;
    }
    const bool fwd = counted && !relay_exhausted(c);
    const uint64_t m = __ballot(fwd);
    uint32_t base = 0;
    const uint32_t lane = threadIdx.x & 63u;
    if (m) {
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        if (lane == leader) base = atomicAdd(a.ws.nsub, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, (int)leader);
    }
    if (counted) relay_send_one(a, i, t, c, base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
}

__global__ void relay_finish_kernel(neb_tx_tunnel* __restrict__ tun, uint32_t ntun, RelayWs ws) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntun) tun[t].message_counter += ws.tun_total[t];
}

__global__ __launch_bounds__(256) void relay_fix_kernel(RelayWs ws, int32_t* __restrict__ fwd_status) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= *ws.nsub) return;
    const int32_t st = ws.sub_status[j];
    if (st != NEB_STATUS_OK) fwd_status[ws.sub_map[j]] = st;
}

}  // namespace neb

extern "C" size_t neb_relay_ws_bytes(uint32_t n, uint32_t ntun, size_t* cub_bytes) {
    size_t c1 = 0, c2 = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, c1, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
    hipcub::DeviceScan::ExclusiveSumByKey(nullptr, c2, (const uint32_t*)nullptr,
                                          hipcub::ConstantInputIterator<uint32_t>(1u), (uint32_t*)nullptr, (int)n);
    *cub_bytes = std::max(c1, c2);
    return neb::relay_ws_layout(n, ntun, *cub_bytes, nullptr, nullptr);
}

extern "C" hipError_t neb_relay_plan(const neb_rx_packet* d_pk, const neb_relay_route* d_route,
                                     const int32_t* d_status, uint32_t n, neb_tx_tunnel* d_tun, uint32_t ntun,
                                     const uint32_t* d_keys, uint32_t max_keys, int alg, uint8_t* d_arena,
                                     int32_t* d_fwd_status, const neb::RelayWs* ws, hipStream_t s) {
    const neb::RelayArgs a{d_pk, d_route, d_status, n, d_tun, ntun, d_keys, max_keys, alg, d_arena, d_fwd_status, *ws};
    int bits = 1;
    while (bits < 32 && (1ull << bits) <= ntun) bits++;  // the keys 0..ntun
    const uint32_t grid = (n + 255u) / 256u;
    if (n <= neb::kRelayPlanSmallMax) {
        auto plan = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(1), dim3(neb::kRelayPlanThreads), 0, s, a, bits); };
        if (n <= neb::kRelayPlanThreads) {
            plan(neb::relay_plan_small_kernel<1, false>);
        } else {
            hipLaunchKernelGGL(neb::relay_mark_kernel, dim3(grid), dim3(256), 0, s, a);
            // the block sort and scans cost by items per thread: 2 up to 2048 packets
            if (n <= 2u * neb::kRelayPlanThreads) plan(neb::relay_plan_small_kernel<2, true>);
            else plan(neb::relay_plan_small_kernel<neb::kRelayPlanItems, true>);
        }
        return hipGetLastError();
    }
    hipError_t e = ntun ? hipMemsetAsync(ws->tun_total, 0, (size_t)ntun * sizeof(uint32_t), s) : hipSuccess;
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(neb::relay_mark_kernel, dim3(grid), dim3(256), 0, s, a);
    size_t cb = ws->cub_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(ws->cub_tmp, cb, ws->key, ws->key_sorted, ws->idx, ws->idx_sorted, (int)n, 0,
                                           bits, s);
    if (e != hipSuccess) return e;
    cb = ws->cub_bytes;
    e = hipcub::DeviceScan::ExclusiveSumByKey(ws->cub_tmp, cb, ws->key_sorted, hipcub::ConstantInputIterator<uint32_t>(1u),
                                              ws->rank, (int)n, hipcub::Equality(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(neb::relay_scatter_kernel, dim3(grid), dim3(256), 0, s, a);
    if (ntun) hipLaunchKernelGGL(neb::relay_finish_kernel, dim3((ntun + 255u) / 256u), dim3(256), 0, s, d_tun, ntun, *ws);
    return hipGetLastError();
}

extern "C" hipError_t neb_relay_fix(const neb::RelayWs* ws, uint32_t n, int32_t* d_fwd_status, hipStream_t s) {
    hipLaunchKernelGGL(neb::relay_fix_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, *ws, d_fwd_status);
    return hipGetLastError();
}
