// report.hpp — device workspace of the RX batch report (report.hip), shared with engine.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"
#include "report_core.hpp"

namespace neb {

// Sort keys are 33 bits wide: a key_id or a relay index, or kReportNoKey for a packet that is not
// sorted, which so ends up behind every packet that is.
constexpr uint64_t kReportNoKey = 1ull << 32;
constexpr int kReportKeyBits = 33;

struct ReportWs {
    // by packet index
    uint64_t* tun_key;    // key_id of an authenticated packet, else kReportNoKey
    uint32_t* tun_idx;    // the packet index
    uint64_t* relay_key;  // relay index of an authenticated Message/Relay packet, else kReportNoKey
    uint32_t* work;       // NEB_WORK_*, 0: not listed
    // by sorted position
    uint64_t* tun_key_s;
    uint32_t* tun_idx_s;
    uint64_t* relay_key_s;
    // n + 1 each: flags and lengths, then their exclusive sums (element n: the totals)
    uint64_t *flag_a, *flag_b, *len;  // work | run head << 32; tunnel head | relay head << 32; wire length
    uint64_t *sum_a, *sum_b, *sum_len;
    uint32_t* run_start;    // sorted position of the r-th run's first packet
    uint32_t* relay_start;  // ... of the r-th relay index's first packet
    uint32_t* ends;         // {authenticated packets, relay packets}: where the sorted keys end
    void* cub_tmp;
    size_t cub_bytes;
};

inline size_t report_ws_layout(uint32_t n, size_t cub_bytes, uint8_t* base, ReportWs* ws) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const size_t m = n ? n : 1;
    ReportWs w{};
    w.tun_key = (uint64_t*)take(m * 8);
    w.tun_key_s = (uint64_t*)take(m * 8);
    w.relay_key = (uint64_t*)take(m * 8);
    w.relay_key_s = (uint64_t*)take(m * 8);
    w.flag_a = (uint64_t*)take((m + 1) * 8);
    w.flag_b = (uint64_t*)take((m + 1) * 8);
    w.len = (uint64_t*)take((m + 1) * 8);
    w.sum_a = (uint64_t*)take((m + 1) * 8);
    w.sum_b = (uint64_t*)take((m + 1) * 8);
    w.sum_len = (uint64_t*)take((m + 1) * 8);
    w.tun_idx = (uint32_t*)take(m * 4);
    w.tun_idx_s = (uint32_t*)take(m * 4);
    w.work = (uint32_t*)take(m * 4);
    w.run_start = (uint32_t*)take(m * 4);
    w.relay_start = (uint32_t*)take(m * 4);
    w.ends = (uint32_t*)take(8);
    w.cub_tmp = take(cub_bytes);
    w.cub_bytes = cub_bytes;
    if (ws) *ws = w;
    return off;
}

struct ReportArgs {
    const neb_rx_packet* pk;
    const int32_t* status;
    const uint8_t* arena;
    const neb_udp_addr* from;
    const uint32_t* pkt_entry;
    neb_rx_run* runs;
    neb_rx_relay_used* relay_used;
    neb_rx_work* work;
    uint64_t* metrics;
    uint32_t* counts;
    uint32_t n, nfrom, relayed;
    ReportWs ws;
};

}  // namespace neb

extern "C" size_t neb_report_ws_bytes(uint32_t n, size_t* cub_bytes);
// Enqueues the whole report on s (a.ws: a workspace laid out for at least a.n packets; a.n != 0).
extern "C" hipError_t neb_report_run(const neb::ReportArgs* a, hipStream_t s);
