// resolve.hip — the index table on the device (neb_index_table_*, neb_rx_resolve_batch; index.cpp
// holds the host half): the lookups readOutsidePackets makes per datagram before it can decrypt
// (outside.go:66-74, :93-106, :201-240), for a whole receive batch in one launch.
//
//   resolve   one lane per packet (idx_resolve_one, index_core.hpp): the header's first 8 bytes, at
//             most two probe chains (the outer index; the inner one behind a terminal relay), the
//             source address against the own networks. It only reads the table.
//   scatter   applies one neb_index_table_update to an image, one thread per slot, fed from pinned
//             staging on the caller's stream.
//
// Visibility. A resolve may run on another stream while a scatter runs, so the two never rely on a
// kernel boundary between them. Every access to a slot, on both sides, is an 8-byte agent-scope
// atomic: such loads are served by the L2 and never by a CU's L1, so no resolve reads a line that
// went stale, and no acquire (an L1 invalidate, microseconds per wave) is needed per probe. The
// scatter writes a record, releases it at agent scope, and only then publishes the tag; a slot's
// record is written once per image (index_core.hpp, IdxSlot), so a lane that has seen the tag reads
// that record and no other. The resolve reads a slot's words in program order: tag, then a, then b.
#include <hip/hip_runtime.h>

#include "../../include/nebula_aead.h"
#include "device_common.hpp"
#include "index_core.hpp"
#include "resolve.hpp"

namespace neb {

struct ResolveArgs {
    const IdxSlot* image;
    uint32_t mask;
    uint32_t n;
    neb_rx_packet* pk;
    const neb_rx_source* src;
    const uint8_t* arena;
    neb_relay_route* route;
    neb_rx_via* via;
    IdxNets nets;  // in the kernel arguments: scanned through the scalar cache, wave-uniformly
};

__global__ __launch_bounds__(256) void idx_resolve_kernel(ResolveArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const neb_rx_packet p = a.pk[i];
    const uint32_t len = idx_rx_len(p);

    bool own = false;
    if (a.src) {  // 20 bytes per lane, five dwords
        const uint32_t* q = reinterpret_cast<const uint32_t*>(a.src + i);
        const uint32_t w[4] = {q[0], q[1], q[2], q[3]};
        const uint32_t family = q[4] & 255u;
        own = family != 0u && idx_own_source(a.nets, family, w);
    }

    // off has no alignment: dword loads where it allows, else the six bytes the rule needs
    const uint8_t* h = a.arena + p.off;
    const bool dwords = (reinterpret_cast<uintptr_t>(h) & 3u) == 0u;
    auto hdr = [&](uint32_t at, uint32_t* w0, uint32_t* w1) {
        const uint8_t* b = h + at;
        if (dwords) {
            *w0 = reinterpret_cast<const uint32_t*>(b)[0];
            *w1 = reinterpret_cast<const uint32_t*>(b)[1];
        } else {
            *w0 = b[0] | ((uint32_t)b[1] << 8);
            *w1 = b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16) | ((uint32_t)b[7] << 24);
        }
    };
    auto look = [&](uint32_t space, uint32_t index, bool want_route, IdxRec* r) {
        return idx_lookup(a.image, a.mask, space, index, LoadAgent{}, want_route, r);
    };
    uint32_t key;
    neb_relay_route route;
    neb_rx_via via;
    idx_resolve_one(len, hdr, look, &key, &route, &via);

    a.pk[i].key_id = key;
    if (own && !(p.len & NEB_RX_OWN_SOURCE)) a.pk[i].len = p.len | NEB_RX_OWN_SOURCE;
    if (a.route) a.route[i] = route;
    if (a.via) a.via[i] = via;
}

__global__ __launch_bounds__(256) void idx_scatter_kernel(IdxSlot* image, const IdxOp* ops, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const IdxOp op = ops[i];
    IdxSlot* s = image + op.slot;
    if (op.tag == kIdxTomb) {
        __hip_atomic_store(&s->tag, kIdxTomb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    __hip_atomic_store(&s->a, op.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s->b, op.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s->tag, op.tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // after a and b
}

}  // namespace neb

extern "C" hipError_t neb_idx_scatter(neb::IdxSlot* image, const neb::IdxOp* ops, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(neb::idx_scatter_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, image, ops, n);
    return hipGetLastError();
}

extern "C" hipError_t neb_idx_resolve(const neb::IdxSlot* image, uint32_t mask, const neb::IdxNets* nets,
                                      neb_rx_packet* d_pk, const neb_rx_source* d_src, uint32_t n,
                                      const uint8_t* d_arena, neb_relay_route* d_route, neb_rx_via* d_via,
                                      hipStream_t s) {
    const neb::ResolveArgs a{image, mask, n, d_pk, d_src, d_arena, d_route, d_via, *nets};
    hipLaunchKernelGGL(neb::idx_resolve_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}
