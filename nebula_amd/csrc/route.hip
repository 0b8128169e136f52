// route.hip — the TX table on the device (neb_tx_table_*, neb_tx_resolve_batch; route.cpp holds the
// host half): the front half of consumeInsidePacket (inside.go:19-121) for a whole batch of TUN
// reads in one launch, in front of neb_tx_seal_batch / neb_tx_seal_via_batch.
//
//   resolve   one lane per TUN read (tx_resolve_one, route_core.hpp): newPacket over the packet's
//             first bytes, the three gates over the own networks, then the host entry of the
//             destination or one probe per route prefix length present, the ECMP bucket, and the
//             gateway's host entry. It only reads the table.
//   scatter   applies one neb_tx_table_update_hosts to an image, one thread per slot, fed from
//             pinned staging on the caller's stream.
//
// Visibility is resolve.hip's: every access to a slot, on both sides, is an 8-byte agent-scope
// atomic, served by the L2 and never by a CU's L1. The scatter writes value and address words,
// then publishes the tag with a release store; a slot's record is written once per image, so a lane
// that has seen the tag reads that record and no other. The resolve reads a slot's words in program
// order: tag, address words, value. The gateway array is written only while its image is the spare
// one, before the switch, so plain loads read it.
#include <hip/hip_runtime.h>

#include "../../include/nebula_aead.h"
#include "device_common.hpp"
#include "route.hpp"
#include "route_core.hpp"

namespace neb {

struct TxResolveArgs {
    const TxSlot* image;
    const TxGw* gws;
    neb_tx_packet* pk;
    const uint8_t* in;
    neb_fw_packet* fw;
    int32_t* status;
    uint32_t mask;
    uint32_t n;
    TxLens lens;  // in the kernel arguments: scanned through the scalar cache, wave-uniformly
    TxOwn own;
};

__global__ __launch_bounds__(256) void tx_resolve_kernel(TxResolveArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t in_off = a.pk[i].in_off;
    const uint32_t len = a.pk[i].len;

    // in_off has no alignment (a virtio header in front leaves it at 2 mod 4): nothing outside
    // [in_off, in_off + len) is read
    const SpanBytes byte(a.in + in_off, len);
    auto look = [&](uint32_t kind, uint32_t family, uint32_t bits, const TxAddr& addr, uint64_t* v) {
        return tx_lookup(a.image, a.mask, kind, family, bits, addr, LoadAgent{}, v);
    };
    auto gw = [&](uint32_t k) { return a.gws[k]; };
    TxResult r;
    tx_resolve_one(len, byte, a.own, a.lens, look, gw, &r);

    a.pk[i].tunnel = r.tunnel;
    if (a.status) a.status[i] = r.status;
    if (a.fw) {  // 48 bytes per lane: three 16-byte stores
        uint4* o = reinterpret_cast<uint4*>(a.fw + i);
        o[0] = make_uint4(r.fw[0], r.fw[1], r.fw[2], r.fw[3]);
        o[1] = make_uint4(r.fw[4], r.fw[5], r.fw[6], r.fw[7]);
        o[2] = make_uint4(r.fw[8], r.fw[9], r.fw[10], r.fw[11]);
    }
}

__global__ __launch_bounds__(256) void tx_scatter_kernel(TxSlot* image, uint32_t mask, const TxOp* ops, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const TxOp op = ops[i];
    if (op.slot > mask) return;
    TxSlot* s = image + op.slot;
    if (op.tag == kTxTomb) {
        __hip_atomic_store(&s->tag, kTxTomb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    __hip_atomic_store(&s->value, op.value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s->addr_lo, op.addr_lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s->addr_hi, op.addr_hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&s->tag, op.tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // after the record
}

}  // namespace neb

extern "C" hipError_t neb_txt_scatter(neb::TxSlot* image, uint32_t mask, const neb::TxOp* ops, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(neb::tx_scatter_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, image, mask, ops, n);
    return hipGetLastError();
}

extern "C" hipError_t neb_txt_resolve(const neb::TxSlot* image, uint32_t mask, const neb::TxGw* gws,
                                      const neb::TxLens* lens, const neb::TxOwn* own, neb_tx_packet* d_pk, uint32_t n,
                                      const uint8_t* d_in, neb_fw_packet* d_fw, int32_t* d_status, hipStream_t s) {
    const neb::TxResolveArgs a{image, gws, d_pk, d_in, d_fw, d_status, mask, n, *lens, *own};
    hipLaunchKernelGGL(neb::tx_resolve_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}
