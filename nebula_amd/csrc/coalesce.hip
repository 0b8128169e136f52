// coalesce.hip — the receive coalescer on the device: opened packets -> TUN writes (TSO / USO
// superpackets), MultiCoalescer.Flush for a whole batch.
//
// The reference walks the sorted batch once with a map of open chains. Here the walk is decomposed
// so that no stage is longer than 64 dependent steps or log2(n) launches:
//   parse     one thread per packet: class, lane, flow hash (coalesce_core.hpp)
//   sort      stable radix sort of indices by counter, then by epoch: the position is "time"
//   barriers  per lane, the running count of unparseable packets: no chain spans two counts
//   flows     stable sort of the data / sealing packets by (lane, flow hash); each packet finds the
//             previous packet with the same 38-byte key in its hash group (the hash only groups)
//   links     can packet q extend a chain that packet p, its flow's previous packet, rides?
//             (every seed comparison of canAppend is an equality or a +1 chain: neighbours suffice)
//   chains    for every data packet as a hypothetical seed, <= 64 steps give the chain's end and
//             the next seed; the real seeds are those reachable from a run's first packet: pointer
//             jumping, log2(n) launches
//   emit      slots by (lane, position): scan -> write index; scan of 16-aligned sizes -> offsets;
//             the fitting prefix; writes[], patched headers, per-packet results
//   gather    the bandwidth kernel: 16 lanes per packet, aligned 16-byte stores, source through
//             load_shifted16
// Grid-wide dependencies are separate launches; nothing spins.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <hipcub/hipcub.hpp>

#include "../../include/nebula_aead.h"
#include "coalesce.hpp"
#include "coalesce_core.hpp"
#include "device_common.hpp"
#include "timing.hpp"

namespace neb {

constexpr uint32_t kCoThreads = 256;
constexpr uint32_t kLwPsh = 1u << 17, kLwLink = 1u << 18, kLwData = 1u << 19, kLwPay = 0x1FFFFu;
constexpr uint64_t kFlowExcluded = 1ull << 33;  // flow sort key: excluded | lane << 32 | hash

struct Co3Sum {
    __host__ __device__ Co3 operator()(const Co3& x, const Co3& y) const {
        Co3 r;
        r.a[0] = x.a[0] + y.a[0];
        r.a[1] = x.a[1] + y.a[1];
        r.a[2] = x.a[2] + y.a[2];
        return r;
    }
};

struct CoArgs {
    const neb_plain_packet* plain;
    const uint8_t* in;
    uint8_t* out;
    uint64_t out_cap;
    neb_tun_write* writes;
    uint32_t* nwrites;
    uint32_t* pkt_write;
    int32_t* pkt_status;
    uint32_t n, max_writes, lanes, hash_mask;
    CoWs ws;
};

__global__ void co_parse_kernel(CoArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const neb_plain_packet pp = a.plain[i];
    CoRec r;
    co_classify(pp, a.in + pp.off, a.lanes, &r);
    uint32_t h = 0;
    if (r.status == NEB_STATUS_OK && r.lane != kCoLanePt && (r.cls == kCoData || r.cls == kCoSeal))
        h = co_flow_hash(a.in + pp.off, r.info) & a.hash_mask;
    a.ws.rec[i] = r;
    a.ws.hash[i] = h;
    a.ws.k0[i] = pp.counter;
    a.ws.i0[i] = i;
}

__global__ void co_epoch_key_kernel(CoArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    a.ws.k0[j] = a.plain[a.ws.i1[j]].epoch;
}

// By position: the barrier scan's input (k0) and the flow sort's key (k1) and value (i0).
__global__ void co_lane_key_kernel(CoArgs a) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t i = a.ws.order[pos];
    const CoRec& r = a.ws.rec[i];
    uint64_t bar = 0, fk = kFlowExcluded;
    if (r.status == NEB_STATUS_OK && r.lane != kCoLanePt) {
        if (r.cls == kCoUnparse) bar = r.lane == kCoLaneTcp ? 1ull << 32 : 1ull;
        if (r.cls == kCoData || r.cls == kCoSeal) fk = ((uint64_t)r.lane << 32) | a.ws.hash[i];
    }
    a.ws.k0[pos] = bar;
    a.ws.k1[pos] = fk;
    a.ws.i0[pos] = pos;
    a.ws.fprev[pos] = kCoNone;
    a.ws.fnext[pos] = kCoNone;
    a.ws.mseed[pos] = kCoNone;
    a.ws.wsize[pos] = 0;
}

// Flow order j (k0 = sorted flow keys): the previous packet of the same hash group with the same
// 38-byte key. Groups with more than one key are rare; the scan then passes the other keys' packets.
__global__ void co_pred_kernel(CoArgs a) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t key = a.ws.k0[j];
    if (key & kFlowExcluded) return;
    const uint32_t pos = a.ws.fpos[j], i = a.ws.order[pos];
    const uint8_t* p = a.in + a.plain[i].off;
    const CoInfo info = a.ws.rec[i].info;
    for (uint32_t jj = j; jj-- > 0;) {
        if (a.ws.k0[jj] != key) break;
        const uint32_t pos2 = a.ws.fpos[jj], i2 = a.ws.order[pos2];
        if (co_flow_equal(a.in + a.plain[i2].off, a.ws.rec[i2].info, p, info)) {
            a.ws.fprev[pos] = pos2;
            a.ws.fnext[pos2] = pos;
            break;
        }
    }
}

__global__ void co_link_kernel(CoArgs a) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t i = a.ws.order[pos];
    const CoRec r = a.ws.rec[i];
    uint32_t lw = 0, reach = 0;
    if (r.status == NEB_STATUS_OK && r.lane != kCoLanePt && (r.cls == kCoData || r.cls == kCoSeal)) {
        const bool tcp = r.lane == kCoLaneTcp;
        lw = r.info.pay_len & kLwPay;
        if (tcp && (r.info.flags & kCoTcpPsh)) lw |= kLwPsh;
        if (r.cls == kCoData) {
            lw |= kLwData;
            const uint32_t pp = a.ws.fprev[pos];
            bool link = false;
            if (pp != kCoNone) {
                const uint32_t i2 = a.ws.order[pp];
                const CoRec r2 = a.ws.rec[i2];
                const uint64_t b1 = a.ws.bar[pp], b2 = a.ws.bar[pos];
                const bool same_bar = tcp ? (b1 >> 32) == (b2 >> 32) : (uint32_t)b1 == (uint32_t)b2;
                link = r2.cls == kCoData && same_bar &&
                       co_link(a.in + a.plain[i2].off, r2.info, a.in + a.plain[i].off, r.info, tcp);
            }
            if (link) lw |= kLwLink;
            reach = !link;
        }
    }
    a.ws.lw[pos] = lw;
    a.ws.reach[pos] = reach;
}

// Every data packet as a hypothetical seed: its chain is decided by the payload lengths, PSH and the
// two caps of the linked packets after it.
__global__ void co_chain_kernel(CoArgs a) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t lw = a.ws.lw[pos];
    uint32_t jump = pos, nseg = 0, total = 0, psh = 0;
    if (lw & kLwData) {
        const uint32_t hdr = a.ws.rec[a.ws.order[pos]].info.hdr_len;
        const uint32_t gso = lw & kLwPay;
        nseg = 1;
        total = gso;
        bool closed = (lw & kLwPsh) != 0;  // PSH on the seed: never open
        uint32_t last = pos, q = a.ws.fnext[pos];
        while (!closed && q != kCoNone) {
            const uint32_t w = a.ws.lw[q];
            if (!(w & kLwLink)) break;
            const uint32_t pl = w & kLwPay;
            if (nseg >= kCoMaxSegs || pl > gso || hdr + total + pl > kCoBufSize) break;
            nseg++;
            total += pl;
            last = q;
            if (w & kLwPsh) psh = 1;
            closed = pl < gso || (w & kLwPsh);
            q = a.ws.fnext[q];
        }
        const uint32_t nx = a.ws.fnext[last];
        // the packet after the chain is the next seed; unless it starts a run itself (already marked)
        if (nx != kCoNone && (a.ws.lw[nx] & kLwLink)) jump = nx;
    }
    a.ws.jump0[pos] = jump;
    a.ws.cnseg[pos] = nseg;
    a.ws.ctotal[pos] = total | (psh << 31);
}

// One round of pointer jumping: seeds mark the seed 2^k chains ahead; jumps double.
__global__ void co_jump_kernel(uint32_t n, const uint32_t* __restrict__ jin, uint32_t* __restrict__ jout,
                               uint32_t* reach) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    const uint32_t j = jin[pos];
    if (j != pos && reach[pos]) reach[j] = 1;
    jout[pos] = jin[j];
}

// Real seeds: name the members of their chains; every slot-creating position counts for its lane.
__global__ void co_member_kernel(CoArgs a) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t i = a.ws.order[pos];
    const CoRec& r = a.ws.rec[i];
    Co3 c{};
    if (r.status == NEB_STATUS_OK) {
        bool slot = true;
        if (r.lane != kCoLanePt && r.cls == kCoData) {
            slot = a.ws.reach[pos] != 0;
            if (slot) {
                const uint32_t nseg = a.ws.cnseg[pos];
                uint32_t q = pos;
                for (uint32_t k = 0; k < nseg && q != kCoNone; k++) {
                    a.ws.mseed[q] = pos;
                    a.ws.midx[q] = k;
                    q = a.ws.fnext[q];
                }
            }
        }
        if (slot) c.a[r.lane] = 1;
    }
    a.ws.sc_in[pos] = c;
}

__device__ inline uint32_t co_total_writes(const CoArgs& a, uint32_t* base_udp, uint32_t* base_pt) {
    const Co3 x = a.ws.sc_out[a.n - 1], y = a.ws.sc_in[a.n - 1];
    const uint32_t t = x.a[0] + y.a[0], u = x.a[1] + y.a[1], p = x.a[2] + y.a[2];
    *base_udp = t;
    *base_pt = t + u;
    return t + u + p;
}

__global__ void co_slot_kernel(CoArgs a) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n) return;
    const Co3 in = a.ws.sc_in[pos];
    uint32_t k = kCoNone;
    if (in.a[0] | in.a[1] | in.a[2]) {
        uint32_t bu, bp;
        co_total_writes(a, &bu, &bp);
        const Co3 ex = a.ws.sc_out[pos];
        k = in.a[0] ? ex.a[0] : in.a[1] ? bu + ex.a[1] : bp + ex.a[2];
        const uint32_t i = a.ws.order[pos];
        const CoRec& r = a.ws.rec[i];
        uint32_t len = a.plain[i].len;
        if (r.lane != kCoLanePt && r.cls == kCoData && a.ws.cnseg[pos] >= 2)
            len = r.info.hdr_len + (a.ws.ctotal[pos] & 0x7FFFFFFFu);
        a.ws.wsize[k] = co_align16(len);
        a.ws.wpos[k] = pos;
    }
    a.ws.wk[pos] = k;
}

__device__ inline bool co_fits(const CoArgs& a, uint32_t k) {
    return k < a.max_writes && a.ws.woff[k] + a.ws.wsize[k] <= a.out_cap;
}

// One thread per write: writes[k], the chain's patched header, and the count of the fitting prefix.
__global__ void co_emit_kernel(CoArgs a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bu, bp;
    const uint32_t W = co_total_writes(a, &bu, &bp);
    if (k == 0 && (W == 0 || !co_fits(a, 0))) *a.nwrites = 0;
    if (k >= W || !co_fits(a, k)) return;
    if (k + 1 == W || !co_fits(a, k + 1)) *a.nwrites = k + 1;
    const uint32_t pos = a.ws.wpos[k], i = a.ws.order[pos];
    const CoRec r = a.ws.rec[i];
    const uint64_t off = a.ws.woff[k];
    const uint32_t nseg = a.ws.cnseg[pos];
    if (r.lane == kCoLanePt || r.cls != kCoData || nseg < 2) {
        co_write_verbatim(&a.writes[k], off, a.plain[i].len, i, r.lane);
        return;
    }
    const bool tcp = r.lane == kCoLaneTcp;
    const uint32_t ct = a.ws.ctotal[pos], total = ct & 0x7FFFFFFFu, hl = r.info.hdr_len;
    co_write_chain(&a.writes[k], off, i, nseg, hl, r.info.ip_hdr_len, total, r.info.pay_len, r.info.v6, tcp);
    uint8_t hdr[100];  // IP 40 + TCP 60 at most
    const uint8_t* src = a.in + a.plain[i].off;
    for (uint32_t b = 0; b < hl; b++) hdr[b] = src[b];
    co_patch_header(hdr, r.info.v6, r.info.ip_hdr_len, hl, total, tcp, ct >> 31);
    uint8_t* dst = a.out + off;
    for (uint32_t b = 0; b < hl; b++) dst[b] = hdr[b];
}

// Per-packet results and the gather's work items.
__global__ void co_result_kernel(CoArgs a) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t i = a.ws.order[pos];
    const CoRec r = a.ws.rec[i];
    CoCopy cp{0, 0, 0, 0};
    uint32_t w = NEB_WRITE_NONE;
    int32_t st = r.status;
    if (st == NEB_STATUS_OK) {
        const bool data = r.lane != kCoLanePt && r.cls == kCoData;
        const uint32_t spos = data ? a.ws.mseed[pos] : pos;
        const uint32_t k = spos < a.n ? a.ws.wk[spos] : kCoNone;
        if (!co_fits(a, k)) {
            st = NEB_STATUS_NO_SPACE;
        } else {
            w = k;
            const neb_plain_packet pp = a.plain[i];
            const bool chain = data && a.ws.cnseg[spos] >= 2;
            cp.src_off = pp.off;
            cp.dst_off = a.ws.woff[k];
            cp.len = pp.len;
            if (chain) {
                const CoRec& sr = a.ws.rec[a.ws.order[spos]];
                cp.src_off += r.info.hdr_len;
                cp.dst_off += sr.info.hdr_len + (uint64_t)a.ws.midx[pos] * sr.info.pay_len;
                cp.len = r.info.pay_len;
            }
            // never leave the write's own slot, whatever the plan says
            if (cp.dst_off + cp.len > a.ws.woff[k] + a.ws.wsize[k]) cp.len = 0;
        }
    }
    a.pkt_write[i] = w;
    a.pkt_status[i] = st;
    a.ws.cp[pos] = cp;
}

// The bandwidth kernel: 16 lanes per packet. Bytes up to the destination's 16-byte boundary and the
// tail go byte by byte; the body is aligned 16-byte stores of two aligned 16-byte loads shifted
// together (load_shifted16: both blocks hold bytes of the packet, so no load leaves it). No LDS.
constexpr uint32_t kCoGatherLanes = 16;
__global__ void __launch_bounds__(kCoThreads) co_gather_kernel(uint32_t n, const CoCopy* __restrict__ cps,
                                                               const uint8_t* __restrict__ in,
                                                               uint8_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pos = t / kCoGatherLanes, l = t % kCoGatherLanes;
    if (pos >= n) return;
    const CoCopy cp = cps[pos];
    if (cp.len == 0) return;
    const uint8_t* s = in + cp.src_off;
    uint8_t* d = out + cp.dst_off;
    const uint32_t L = cp.len;
    const uint32_t head = min(L, (16u - ((uint32_t)reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);
    if (l < head) d[l] = s[l];
    const uint32_t nb = (L - head) / 16u;
    const uint8_t* sb = s + head;
    uint4* db = reinterpret_cast<uint4*>(d + head);
    const bool src_aligned = ((uint32_t)reinterpret_cast<uintptr_t>(sb) & 15u) == 0u;
    if (src_aligned) {
        const uint4* s4 = reinterpret_cast<const uint4*>(sb);
        for (uint32_t c = l; c < nb; c += kCoGatherLanes) db[c] = s4[c];
    } else {
        for (uint32_t c = l; c < nb; c += kCoGatherLanes) db[c] = load_shifted16(sb + 16u * c);
    }
    const uint32_t t0 = head + 16u * nb;
    if (l < L - t0) d[t0 + l] = s[t0 + l];
}

__global__ void co_plain_from_wire_kernel(const neb_rx_packet* pk, const int32_t* status, const uint64_t* epoch,
                                          uint32_t nepoch, uint32_t n, const uint8_t* arena, neb_plain_packet* plain) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    neb_plain_packet o;
    co_plain_from_wire(pk[i], status[i], arena, epoch, nepoch, &o);
    plain[i] = o;
}

}  // namespace neb

extern "C" size_t neb_co_ws_bytes(uint32_t n, size_t* cub_bytes) {
    size_t c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, c1, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
    hipcub::DeviceScan::InclusiveSum(nullptr, c2, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n);
    hipcub::DeviceScan::ExclusiveSum(nullptr, c3, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n);
    hipcub::DeviceScan::ExclusiveScan(nullptr, c4, (const neb::Co3*)nullptr, (neb::Co3*)nullptr, neb::Co3Sum(),
                                      neb::Co3{}, (int)n);
    *cub_bytes = std::max(std::max(c1, c2), std::max(c3, c4));
    return neb::co_ws_layout(n, *cub_bytes, nullptr, nullptr);
}

extern "C" hipError_t neb_co_run(const neb_plain_packet* d_plain, uint32_t n, const uint8_t* d_in, uint8_t* d_out,
                                 uint64_t out_cap, neb_tun_write* d_writes, uint32_t max_writes, uint32_t* d_nwrites,
                                 uint32_t* d_pkt_write, int32_t* d_pkt_status, uint32_t lanes, uint32_t hash_bits,
                                 const neb::CoWs* ws, hipStream_t s) {
    using namespace neb;
    CoArgs a{};
    a.plain = d_plain;
    a.in = d_in;
    a.out = d_out;
    a.out_cap = out_cap;
    a.writes = d_writes;
    a.nwrites = d_nwrites;
    a.pkt_write = d_pkt_write;
    a.pkt_status = d_pkt_status;
    a.n = n;
    a.max_writes = max_writes;
    a.lanes = lanes;
    a.hash_mask = hash_bits >= 32 ? 0xFFFFFFFFu : (1u << hash_bits) - 1u;
    a.ws = *ws;
    const dim3 tpb(kCoThreads), grid((n + kCoThreads - 1) / kCoThreads);
    hipError_t e;
    size_t cb;
#define CO_LAUNCH(kernel) hipLaunchKernelGGL(kernel, grid, tpb, 0, s, a)
    // parse, then the stable sort by (epoch, counter): least significant key first
    CO_LAUNCH(co_parse_kernel);
    cb = ws->cub_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(ws->cub_tmp, cb, ws->k0, ws->k1, ws->i0, ws->i1, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    CO_LAUNCH(co_epoch_key_kernel);
    cb = ws->cub_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(ws->cub_tmp, cb, ws->k0, ws->k1, ws->i1, ws->order, (int)n, 0, 64, s);
    if (e != hipSuccess) return e;
    // barriers; per-flow order
    CO_LAUNCH(co_lane_key_kernel);
    cb = ws->cub_bytes;
    e = hipcub::DeviceScan::InclusiveSum(ws->cub_tmp, cb, ws->k0, ws->bar, (int)n, s);
    if (e != hipSuccess) return e;
    cb = ws->cub_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(ws->cub_tmp, cb, ws->k1, ws->k0, ws->i0, ws->fpos, (int)n, 0, 34, s);
    if (e != hipSuccess) return e;
    CO_LAUNCH(co_pred_kernel);
    // links, chains, the real seeds
    CO_LAUNCH(co_link_kernel);
    CO_LAUNCH(co_chain_kernel);
    uint32_t* jin = ws->jump0;
    uint32_t* jout = ws->jump1;
    for (uint32_t span = 1; span < n; span <<= 1) {
        hipLaunchKernelGGL(co_jump_kernel, grid, tpb, 0, s, n, jin, jout, ws->reach);
        std::swap(jin, jout);
    }
    // emit
    CO_LAUNCH(co_member_kernel);
    cb = ws->cub_bytes;
    e = hipcub::DeviceScan::ExclusiveScan(ws->cub_tmp, cb, ws->sc_in, ws->sc_out, Co3Sum(), Co3{}, (int)n, s);
    if (e != hipSuccess) return e;
    CO_LAUNCH(co_slot_kernel);
    cb = ws->cub_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(ws->cub_tmp, cb, ws->wsize, ws->woff, (int)n, s);
    if (e != hipSuccess) return e;
    CO_LAUNCH(co_emit_kernel);
    CO_LAUNCH(co_result_kernel);
    // gather
    const uint64_t gthreads = (uint64_t)n * kCoGatherLanes;
    // the call's dominant kernel: an armed neb_time_next_kernel pair is bound to it
    e = launch_bound(co_gather_kernel, dim3((uint32_t)((gthreads + kCoThreads - 1) / kCoThreads)), tpb, s, nullptr, n,
                     (const CoCopy*)ws->cp, d_in, d_out);
#undef CO_LAUNCH
    return e != hipSuccess ? e : hipGetLastError();
}

extern "C" hipError_t neb_co_plain_from_wire(const neb_rx_packet* d_pk, const int32_t* d_status,
                                             const uint64_t* d_epoch, uint32_t nepoch, uint32_t n,
                                             const uint8_t* d_arena, neb_plain_packet* d_plain, hipStream_t s) {
    hipLaunchKernelGGL(neb::co_plain_from_wire_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, d_pk, d_status,
                       d_epoch, nepoch, n, d_arena, d_plain);
    return hipGetLastError();
}
