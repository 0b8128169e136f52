// peer.hip — the RX inner resolve on the device (neb_rx_inner_batch; peer.cpp holds the host half):
// what handleOutsideMessagePacket does between Decrypt and Commit (outside.go:474-494), short of the
// rules and conntrack, for a whole opened batch in one launch, in neb_rx_plain_from_wire's place.
//
//   inner   one lane per packet (peer_inner_one, peer_core.hpp): the commit rule over the 16-byte
//           header, newPacket(incoming) over the plaintext's first bytes, one probe per prefix
//           length present among the tunnel's entries, the scan of the routable set, then the
//           commit record and the firewall's packet. It only reads the table.
//
// The images are written by route.hip's scatter and read as route.hip reads them: every access to a
// slot is an 8-byte agent-scope atomic, tag first, then the address words, then the value.
#include <hip/hip_runtime.h>

#include "../../include/nebula_aead.h"
#include "device_common.hpp"
#include "peer.hpp"
#include "peer_core.hpp"

namespace neb {

struct PeerInnerArgs {
    const TxSlot* image;
    const neb_rx_packet* pk;
    const int32_t* status;
    const uint64_t* epoch;
    const uint8_t* arena;
    neb_plain_packet* plain;
    neb_fw_packet* fw;
    int32_t* inner_status;
    uint32_t mask;
    uint32_t nepoch;
    uint32_t n;
    TxLens lens;  // in the kernel arguments: scanned through the scalar cache, wave-uniformly
    PeerRoutable routable;
};
static_assert(sizeof(PeerInnerArgs) < 4096, "HIP's limit for kernel arguments");

__global__ __launch_bounds__(256) void peer_inner_kernel(PeerInnerArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const neb_rx_packet pk = a.pk[i];
    const uint32_t len = pk.len & ~NEB_RX_OWN_SOURCE;

    // the arena's base and off have no alignment: two spans, the header and the plaintext, so that no
    // dword read reaches into the tag or past the packet (a packet under 32 bytes is not read at all)
    const uint8_t* h = a.arena + pk.off;
    const SpanBytes hdr(h, len >= 32u ? 16u : 0u), body(h + 16, len >= 32u ? len - 32u : 0u);
    auto epoch = [&](uint32_t k) { return a.epoch[k]; };
    auto look = [&](uint32_t family, uint32_t bits, const TxAddr& addr, uint64_t* v) {
        uint32_t s, probes;
        if (!peer_find(a.image, a.mask, pk.key_id, family, bits, addr, LoadAgent{}, &s, &probes)) return false;
        *v = LoadAgent{}(&a.image[s].value);
        return true;
    };
    PeerResult r;
    peer_inner_one(pk.off, len, pk.key_id, a.status[i], a.nepoch, hdr, body, epoch, a.lens, a.routable, look, &r);

    uint4* o = reinterpret_cast<uint4*>(a.plain + i);  // 32 bytes per lane: two 16-byte stores
    o[0] = make_uint4(r.plain[0], r.plain[1], r.plain[2], r.plain[3]);
    o[1] = make_uint4(r.plain[4], r.plain[5], r.plain[6], r.plain[7]);
    if (a.inner_status) a.inner_status[i] = r.status;
    if (a.fw) {  // 48 bytes per lane: three 16-byte stores
        uint4* f = reinterpret_cast<uint4*>(a.fw + i);
        f[0] = make_uint4(r.fw[0], r.fw[1], r.fw[2], r.fw[3]);
        f[1] = make_uint4(r.fw[4], r.fw[5], r.fw[6], r.fw[7]);
        f[2] = make_uint4(r.fw[8], r.fw[9], r.fw[10], r.fw[11]);
    }
}

}  // namespace neb

extern "C" hipError_t neb_peer_inner(const neb::TxSlot* image, uint32_t mask, const neb::TxLens* lens,
                                     const neb::PeerRoutable* routable, const neb_rx_packet* d_pk,
                                     const int32_t* d_status, const uint64_t* d_epoch, uint32_t nepoch, uint32_t n,
                                     const uint8_t* d_arena, neb_plain_packet* d_plain, neb_fw_packet* d_fw,
                                     int32_t* d_inner_status, hipStream_t s) {
    const neb::PeerInnerArgs a{image, d_pk, d_status, d_epoch, d_arena, d_plain, d_fw, d_inner_status, mask, nepoch, n, *lens, *routable};
    hipLaunchKernelGGL(neb::peer_inner_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}
