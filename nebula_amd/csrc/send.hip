// send.hip — the TX send plan on the device: sealed wires -> sendmmsg entries with UDP_SEGMENT runs,
// WriteBatch's packing loop for a whole batch.
//
// The reference plans run after run: where one run ends decides where the next starts. Here the
// walk is decomposed (rules: send_core.hpp). A routable wire starts a hard segment where no run can
// continue whatever came before; inside a hard segment lengths never increase, so it is a row of
// plateaus of equal length, and all that one plateau passes to the next is one bit: did its last
// run take the next plateau's first packet?
//   classify  one thread per wire slot: class, destination (one neb_udp_addr load), length
//   scan 1    exclusive {max, sum}: the previous wire that is not absent; the routable rank
//   boundary  hard segments and plateau starts against that previous wire
//   scan 2    inclusive max: the rank at which each wire's plateau starts
//   function  at a plateau's first wire, the plateau before it as a function {0,1} -> {0,1}
//   scan 3    inclusive, under composition: every plateau's bit
//   starts    which plateau positions start a run
//   scan 4    inclusive sum: the entry of every wire
//   emit      iov[], wire_entry[], send_status[]; every entry's first rank and destination
//   entries   one thread per entry: niov from the next entry's first rank, bytes, seg_size; the counts
// Six kernels of this file and four hipcub scans: ten launches, 14 kernels with the state
// initialisation each scan launches inside. Grid-wide dependencies are separate launches; nothing
// spins. Every launch covers max_wires slots: *nwires is read on the device, and slots past it are
// absent.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <hipcub/hipcub.hpp>

#include "../../include/nebula_aead.h"
#include "send.hpp"
#include "send_core.hpp"

namespace neb {

constexpr uint32_t kSendThreads = 256;
constexpr uint32_t kSendFlagHard = 1u, kSendFlagPlateau = 2u;

struct SendPrevOp {
    __host__ __device__ SendPrev operator()(const SendPrev& x, const SendPrev& y) const {
        return SendPrev{x.last > y.last ? x.last : y.last, x.rank + y.rank};
    }
};
struct SendFnOp {  // x covers the earlier wires
    __host__ __device__ uint32_t operator()(uint32_t x, uint32_t y) const { return send_fn_compose(x, y); }
};

__device__ inline uint32_t send_nwires(const SendArgs& a) {
    const uint32_t nw = *a.nwires;
    return nw < a.n ? nw : a.n;
}

__global__ void __launch_bounds__(kSendThreads) send_classify_kernel(SendArgs a) {
    const uint32_t i = blockIdx.x * kSendThreads + threadIdx.x;
    if (i >= a.n) return;
    SendRec r{};
    if (i < send_nwires(a))
        send_classify(a.wires[i], a.wire_status[i], a.packets, a.npackets, a.via, a.remote, a.ntunnels, a.socket_v4, &r);
    a.ws.rec[i] = r;
    a.ws.p_in[i] = SendPrev{r.cls != kSendAbsent ? i + 1u : 0u, r.cls == kSendRoutable ? 1u : 0u};
}

__global__ void __launch_bounds__(kSendThreads) send_boundary_kernel(SendArgs a) {
    const uint32_t i = blockIdx.x * kSendThreads + threadIdx.x;
    if (i >= a.n) return;
    const SendRec r = a.ws.rec[i];
    uint32_t flags = 0, ps = 0;
    if (r.cls == kSendRoutable) {
        const SendPrev p = a.ws.p_out[i];
        SendRec prev{};
        if (p.last) prev = a.ws.rec[p.last - 1u];
        if (send_hard(p.last != 0u, prev, r, p.rank, a.chunk_packets)) flags = kSendFlagHard | kSendFlagPlateau;
        else if (prev.len != r.len) flags = kSendFlagPlateau;
        if (flags) ps = p.rank;
    }
    a.ws.flags[i] = flags;
    a.ws.ps_in[i] = ps;
}

__global__ void __launch_bounds__(kSendThreads) send_function_kernel(SendArgs a) {
    const uint32_t i = blockIdx.x * kSendThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t flags = a.ws.flags[i];
    uint32_t fn = kSendFnIdentity;
    if (flags & kSendFlagHard) {
        fn = kSendFnZero;
    } else if (flags & kSendFlagPlateau) {
        // not hard: the previous wire is routable, of the same hard segment, and ends its plateau
        const SendPrev p = a.ws.p_out[i];
        const uint32_t pi = p.last - 1u;
        fn = send_plateau_fn(p.rank - a.ws.ps_out[pi], a.ws.rec[pi].len, a.ws.rec[i].len, a.max_segments);
    }
    a.ws.fn_in[i] = fn;
}

__global__ void __launch_bounds__(kSendThreads) send_start_kernel(SendArgs a) {
    const uint32_t i = blockIdx.x * kSendThreads + threadIdx.x;
    if (i >= a.n) return;
    uint32_t st = 0;
    if (a.ws.p_in[i].rank) {  // routable
        const uint32_t t = a.ws.p_out[i].rank - a.ws.ps_out[i], o = a.ws.fn_out[i] & 1u;
        st = send_run_start(t, o, send_run_cap(a.ws.rec[i].len, a.max_segments));
    }
    a.ws.st_in[i] = st;
}

// Per wire: its iovec, its entry, its status; a run's first wire names the entry's first rank.
__global__ void __launch_bounds__(kSendThreads) send_emit_kernel(SendArgs a) {
    const uint32_t i = blockIdx.x * kSendThreads + threadIdx.x;
    if (i >= send_nwires(a)) return;
    const SendRec r = a.ws.rec[i];
    uint32_t e = NEB_SEND_NONE;
    if (r.cls == kSendRoutable) {
        const uint32_t rank = a.ws.p_out[i].rank;
        e = a.ws.st_out[i] - 1u;
        a.iov[rank] = neb_send_iov{a.wires[i].out_off, r.len, i};
        if (a.ws.st_in[i]) {
            a.ws.efirst[e] = rank;
            a.ws.edst[e] = r.dst;
        }
    }
    a.wire_entry[i] = e;
    a.send_status[i] = send_status_of(r.cls);
}

// Per entry: the ranks up to the next entry's first are its iovecs.
__global__ void __launch_bounds__(kSendThreads) send_entry_kernel(SendArgs a) {
    const uint32_t e = blockIdx.x * kSendThreads + threadIdx.x;
    const uint32_t R = a.ws.p_out[a.n - 1u].rank + a.ws.p_in[a.n - 1u].rank, E = a.ws.st_out[a.n - 1u];
    if (e == 0) {
        *a.niov = R;
        *a.nentries = E;
    }
    if (e >= E) return;
    const uint32_t first = a.ws.efirst[e], end = e + 1u < E ? a.ws.efirst[e + 1u] : R;
    const uint32_t cnt = end - first, len0 = a.iov[first].len, last = a.iov[end - 1u].len;
    a.entries[e] = neb_send_entry{first, (uint16_t)cnt, (uint16_t)(cnt >= 2u ? len0 : 0u), a.ws.edst[e],
                                  len0 * (cnt - 1u) + last};
}

}  // namespace neb

extern "C" size_t neb_send_ws_bytes(uint32_t n, size_t* cub_bytes) {
    using namespace neb;
    size_t c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    hipcub::DeviceScan::ExclusiveScan(nullptr, c1, (const SendPrev*)nullptr, (SendPrev*)nullptr, SendPrevOp(), SendPrev{0, 0},
                                      (int)n);
    hipcub::DeviceScan::InclusiveScan(nullptr, c2, (const uint32_t*)nullptr, (uint32_t*)nullptr, hipcub::Max(), (int)n);
    hipcub::DeviceScan::InclusiveScan(nullptr, c3, (const uint32_t*)nullptr, (uint32_t*)nullptr, SendFnOp(), (int)n);
    hipcub::DeviceScan::InclusiveSum(nullptr, c4, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
    *cub_bytes = std::max(std::max(c1, c2), std::max(c3, c4));
    return send_ws_layout(n, *cub_bytes, nullptr, nullptr);
}

extern "C" hipError_t neb_send_run(const neb::SendArgs* args, hipStream_t s) {
    using namespace neb;
    const SendArgs& a = *args;
    const SendWs& ws = a.ws;
    const int n = (int)a.n;
    const dim3 tpb(kSendThreads), grid((a.n + kSendThreads - 1) / kSendThreads);
    hipError_t e;
    size_t cb;
#define SEND_LAUNCH(kernel) hipLaunchKernelGGL(kernel, grid, tpb, 0, s, a)
    SEND_LAUNCH(send_classify_kernel);
    cb = ws.cub_bytes;
    e = hipcub::DeviceScan::ExclusiveScan(ws.cub_tmp, cb, ws.p_in, ws.p_out, SendPrevOp(), SendPrev{0, 0}, n, s);
    if (e != hipSuccess) return e;
    SEND_LAUNCH(send_boundary_kernel);
    cb = ws.cub_bytes;
    e = hipcub::DeviceScan::InclusiveScan(ws.cub_tmp, cb, ws.ps_in, ws.ps_out, hipcub::Max(), n, s);
    if (e != hipSuccess) return e;
    SEND_LAUNCH(send_function_kernel);
    cb = ws.cub_bytes;
    e = hipcub::DeviceScan::InclusiveScan(ws.cub_tmp, cb, ws.fn_in, ws.fn_out, SendFnOp(), n, s);
    if (e != hipSuccess) return e;
    SEND_LAUNCH(send_start_kernel);
    cb = ws.cub_bytes;
    e = hipcub::DeviceScan::InclusiveSum(ws.cub_tmp, cb, ws.st_in, ws.st_out, n, s);
    if (e != hipSuccess) return e;
    SEND_LAUNCH(send_emit_kernel);
    SEND_LAUNCH(send_entry_kernel);
#undef SEND_LAUNCH
    return hipGetLastError();
}
