// conntrack.hip — the connection table on the device (neb_conntrack_*; conntrack.cpp holds the host
// half, conntrack_core.hpp the rules): firewall.Conntrack.Conns for whole TX and RX batches, between
// the resolves that emit firewall.Packet and the coalescer or the seal.
//
//   lookup   one lane per packet: inConns. Probes 64-byte slots, refreshes Expires with an atomic max
//            on a HIT, stores the verdict byte and the hold marks, a 0/1 flag for the scan, and adds
//            the verdict counts once per wave
//   scan     exclusive sum of the flags: where each MISS / STALE packet goes in the work list
//   scatter  one lane per packet: the work-list entries in ascending packet order, and the counts
//   claim    one lane per key: addConn's probe; an EMPTY slot is claimed with one compare-and-swap, a
//            copy of a key recognises its claimer by the claimer's input, never by the slot's words
//   settle   the second launch of the same add: CLAIMED -> SETTLED, the batch index out of meta; a claimer
//            that came too late for the last place buries its slot, and its copies follow it
//   evict    one lane per key
//   rehash   one lane per slot of the old image: compaction into a cleared one
//
// Every access to a slot or a counter is an 8-byte agent-scope atomic, as in the other tables: served
// by the L2, never by a CU's L1, so no launch needs a fence per element. What one launch must see of
// another comes by the launch boundary (claim -> settle, add -> lookup on one stream); what a lookup on
// another stream sees meanwhile is a whole state word. Nothing spins and no lane waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <hipcub/hipcub.hpp>

#include "../../include/nebula_aead.h"
#include "conntrack.hpp"
#include "conntrack_core.hpp"

namespace neb {

constexpr uint32_t kCtThreads = 256;

struct CtAgentMem {
    __device__ __forceinline__ uint64_t load(const uint64_t* p) const {
        const uint64_t v = __hip_atomic_load(const_cast<uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads in program order
        return v;
    }
    __device__ __forceinline__ void store(uint64_t* p, uint64_t v) const {
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the words a SETTLED state stands for were stored by the launch before: nothing to release
    __device__ __forceinline__ void store_release(uint64_t* p, uint64_t v) const { store(p, v); }
    __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) const {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
    __device__ __forceinline__ uint64_t fetch_add(uint64_t* p, uint64_t v) const {
        return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t fetch_sub(uint64_t* p, uint64_t v) const {
        return __hip_atomic_fetch_add(p, 0ull - v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ uint64_t fetch_max(uint64_t* p, uint64_t v) const {
        return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The 48 bytes of a firewall packet: three 16-byte loads.
struct CtFw {
    uint4 a, b, c;
};
__device__ __forceinline__ CtFw ct_load_fw(const neb_fw_packet* fw) {
    const uint4* f = reinterpret_cast<const uint4*>(fw);
    return CtFw{f[0], f[1], f[2]};
}
__device__ __forceinline__ CtKey ct_key_of_fw(const CtFw& f) {
    const uint64_t q[6] = {f.a.x | ((uint64_t)f.a.y << 32), f.a.z | ((uint64_t)f.a.w << 32), f.b.x | ((uint64_t)f.b.y << 32),
                           f.b.z | ((uint64_t)f.b.w << 32), f.c.x | ((uint64_t)f.c.y << 32), f.c.z | ((uint64_t)f.c.w << 32)};
    return ct_key_from_words(q);
}

__global__ void __launch_bounds__(kCtThreads) conntrack_lookup_kernel(CtLookupArgs a) {
    const uint32_t i = blockIdx.x * kCtThreads + threadIdx.x;
    uint32_t v = NEB_CT_NONE;
    if (i < a.n) {
        if (a.status[i] == NEB_STATUS_OK) {
            v = ct_lookup_one(a.slots, a.p, a.version, a.now, ct_key_of_fw(ct_load_fw(a.fw + i)), CtAgentMem{});
            if (v != NEB_CT_HIT && (a.plain || a.tx)) {
                if (a.plain) a.plain[i].flags |= NEB_PLAIN_SKIP;
                if (a.tx) a.tx[i].tunnel = NEB_TX_NO_TUNNEL;
                a.status[i] = NEB_STATUS_FW_HELD;
            }
        }
        a.verdict[i] = (uint8_t)v;
        a.ws.flag[i] = v > NEB_CT_HIT ? 1u : 0u;
    }
    // the counts: one atomic per wave and kind that occurred (steady traffic: one, the hits)
    const uint32_t code = v & 0x7Fu;
    const uint32_t hits = __popcll(__ballot(code == NEB_CT_HIT)), misses = __popcll(__ballot(code == NEB_CT_MISS)),
                   stales = __popcll(__ballot(code == NEB_CT_STALE));
    if (__lane_id() == __ffsll((unsigned long long)__ballot(1)) - 1) {
        const CtAgentMem m;
        if (hits) m.fetch_add(&a.ws.acc[0], hits);
        if (misses) m.fetch_add(&a.ws.acc[1], misses);
        if (stales) m.fetch_add(&a.ws.acc[2], stales);
    }
}

__global__ void __launch_bounds__(kCtThreads) conntrack_scatter_kernel(CtLookupArgs a) {
    const uint32_t i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t flag = a.ws.flag[i], pos = a.ws.pos[i];
    if (flag && pos < a.work_cap) {  // 64 bytes: four 16-byte stores
        const CtFw f = ct_load_fw(a.fw + i);
        uint4* o = reinterpret_cast<uint4*>(a.work + pos);
        o[0] = make_uint4(i, a.verdict[i], f.a.x, f.a.y);
        o[1] = make_uint4(f.a.z, f.a.w, f.b.x, f.b.y);
        o[2] = make_uint4(f.b.z, f.b.w, f.c.x, f.c.y);
        o[3] = make_uint4(f.c.z, f.c.w, 0u, 0u);
    }
    if (i + 1u == a.n) {  // the totals, and the accumulators back to zero for the next call
        const CtAgentMem m;
        for (int k = 0; k < 3; k++) {
            a.counts[k] = (uint32_t)m.load(&a.ws.acc[k]);
            m.store(&a.ws.acc[k], 0);
        }
        a.counts[3] = pos + flag;
    }
}

__global__ void __launch_bounds__(kCtThreads) conntrack_claim_kernel(CtAddArgs a) {
    const uint32_t i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= a.n) return;
    auto key_of = [&](uint32_t j) { return ct_key_of_fw(ct_load_fw(a.keys + (j < a.n ? j : i))); };
    const CtAdd r = ct_add_claim(a.slots, &a.counters[0], a.p, a.version, a.now, i, key_of(i), a.incoming[i], key_of, CtAgentMem{});
    uint32_t* o = reinterpret_cast<uint32_t*>(a.result + i);
    o[0] = r.code;
    o[1] = r.slot;
}

__global__ void __launch_bounds__(kCtThreads) conntrack_settle_kernel(CtAddArgs a) {
    const uint32_t i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= a.n) return;
    uint32_t* o = reinterpret_cast<uint32_t*>(a.result + i);
    const CtAdd r{o[0], o[1]};
    if (r.code != NEB_CT_FULL && r.slot > a.p.mask) return;  // not the first launch's
    // another element's code: written by the first launch and perhaps again by this one (one word)
    auto code_of = [&](uint32_t j) {
        return __hip_atomic_load(reinterpret_cast<uint32_t*>(a.result + (j < a.n ? j : i)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const CtAdd f = ct_add_settle(a.slots, a.counters, r, code_of, CtAgentMem{});
    if (f.code != r.code) {
        __hip_atomic_store(&o[0], f.code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o[1] = f.slot;
    }
}

__global__ void __launch_bounds__(kCtThreads) conntrack_evict_kernel(CtEvictArgs a) {
    const uint32_t i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= a.n) return;
    a.remaining[i] = ct_evict_one(a.slots, a.counters, a.p, a.now, a.force != 0u, ct_key_of_fw(ct_load_fw(a.keys + i)), CtAgentMem{});
}

__global__ void __launch_bounds__(kCtThreads) conntrack_rehash_kernel(const CtSlot* from, CtSlot* to, uint64_t* counters, CtParams p) {
    const uint32_t i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i == 0u) CtAgentMem{}.store(&counters[1], 0);
    if (i <= p.mask) ct_rehash_one(&from[i], to, p, CtAgentMem{});
}

inline dim3 ct_grid(uint32_t n) { return dim3((n + kCtThreads - 1u) / kCtThreads); }

}  // namespace neb

extern "C" size_t neb_ct_ws_bytes(uint32_t n, size_t* cub_bytes) {
    size_t c = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, c, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n ? n : 1u));
    *cub_bytes = std::max(c, (size_t)256);
    return neb::ct_ws_layout(n, *cub_bytes, nullptr, nullptr);
}

extern "C" hipError_t neb_ct_lookup(const neb::CtLookupArgs* args, hipStream_t s) {
    using namespace neb;
    const CtLookupArgs& a = *args;
    hipLaunchKernelGGL(conntrack_lookup_kernel, ct_grid(a.n), dim3(kCtThreads), 0, s, a);
    size_t cb = a.ws.cub_bytes;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(a.ws.cub_tmp, cb, a.ws.flag, a.ws.pos, (int)a.n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conntrack_scatter_kernel, ct_grid(a.n), dim3(kCtThreads), 0, s, a);
    return hipGetLastError();
}

extern "C" hipError_t neb_ct_add(const neb::CtAddArgs* args, hipStream_t s) {
    using namespace neb;
    hipLaunchKernelGGL(conntrack_claim_kernel, ct_grid(args->n), dim3(kCtThreads), 0, s, *args);
    hipLaunchKernelGGL(conntrack_settle_kernel, ct_grid(args->n), dim3(kCtThreads), 0, s, *args);
    return hipGetLastError();
}

extern "C" hipError_t neb_ct_evict(const neb::CtEvictArgs* args, hipStream_t s) {
    using namespace neb;
    hipLaunchKernelGGL(conntrack_evict_kernel, ct_grid(args->n), dim3(kCtThreads), 0, s, *args);
    return hipGetLastError();
}

extern "C" hipError_t neb_ct_rehash(const neb::CtSlot* from, neb::CtSlot* to, uint64_t* counters, const neb::CtParams* p,
                                    hipStream_t s) {
    using namespace neb;
    hipLaunchKernelGGL(conntrack_rehash_kernel, ct_grid(p->mask + 1u), dim3(kCtThreads), 0, s, from, to, counters, *p);
    return hipGetLastError();
}
