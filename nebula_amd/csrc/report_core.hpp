// report_core.hpp — the rules of the RX batch report, shared by the host form (report.cpp), the
// device form (report.hip) and the sanitizer program (tests/sanitize_report). Plain C++17; compiles
// with g++ alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   readOutsidePackets         outside.go:30-189     the order of the drops and of the metrics
//   handleOutsideRelayPacket   outside.go:191-200    roaming, In and RelayUsed of a verified relay packet
//   newMessageMetrics          message_metrics.go:52-77   the rows of messages.rx.*
// The headerless conditions below are the receive gate's (rxwin.hpp, neb_rx_wire_gate), in its order.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nebula_aead.h"

#if defined(__HIPCC__)
#define NEB_REPORT_HD __host__ __device__
#else
#define NEB_REPORT_HD
#endif

namespace neb {

static_assert(sizeof(neb_rx_run) == 40 && offsetof(neb_rx_run, from) == 20, "");
static_assert(sizeof(neb_rx_relay_used) == 8 && sizeof(neb_rx_work) == 8 && sizeof(neb_udp_addr) == 20, "");

constexpr uint32_t kReportMetrics = NEB_REPORT_NMETRICS;
constexpr uint32_t kReportNoSlot = 0xFFFFFFFFu;

// What the report needs of a packet's header: type, subtype and the remote index. `has` is false
// below 16 bytes, where nothing of the header is read.
struct ReportHeader {
    bool has;
    uint32_t ver, type, sub, index;
};
NEB_REPORT_HD inline ReportHeader report_header(const uint8_t* h, uint32_t len) {
    ReportHeader r{};
    if (len < 16u) return r;
    r.has = true;
    r.ver = h[0] >> 4, r.type = h[0] & 15u, r.sub = h[1];
    r.index = (uint32_t)h[4] << 24 | (uint32_t)h[5] << 16 | (uint32_t)h[6] << 8 | h[7];
    return r;
}

// IsValidSubType (header.go:192-205), as the gate has it.
NEB_REPORT_HD inline bool report_valid_subtype(uint32_t type, uint32_t sub) {
    return (type == 1u || type == 4u) ? sub <= 1u : (type == 0u || (type >= 2u && type <= 6u)) && sub == 0u;
}

// The packet reached `if h.Type != header.Message { Rx(...) }` (outside.go:77): parsed, version 1, a
// valid subtype, and not refused for its own source (which a relayed packet never is).
NEB_REPORT_HD inline bool report_past_gates(const ReportHeader& h, uint32_t raw_len, bool relayed) {
    return h.has && h.ver == 1u && report_valid_subtype(h.type, h.sub) && (relayed || !(raw_len & NEB_RX_OWN_SOURCE));
}

// The row of messages.rx.* a non-Message packet past the gates counts in. Control has no row in
// newMessageMetrics, so Rx() sends it to rx.other.
NEB_REPORT_HD inline uint32_t report_rx_slot(uint32_t type, uint32_t sub) {
    switch (type) {
        case 0u: return NEB_METRIC_RX_HANDSHAKE;
        case 2u: return NEB_METRIC_RX_RECV_ERROR;
        case 3u: return NEB_METRIC_RX_LIGHTHOUSE;
        case 4u: return sub == 0u ? NEB_METRIC_RX_TEST_REQUEST : NEB_METRIC_RX_TEST_RESPONSE;
        case 5u: return NEB_METRIC_RX_CLOSE_TUNNEL;
        default: return NEB_METRIC_RX_OTHER;
    }
}

// Everything the report takes from one packet.
struct ReportPacket {
    uint32_t len;         // without NEB_RX_OWN_SOURCE
    uint32_t rx_slot;     // kReportNoSlot: no Rx(type, subtype)
    uint32_t status_slot; // kReportNoSlot, or NEB_METRIC_OPENED / _AUTH_FAILED / _REPLAY / _NO_TUNNEL
    uint32_t work;        // 0: not on the work list, else NEB_WORK_*
    uint32_t relay_index; // when relay
    bool invalid;         // counts in rx.invalid
    bool auth;            // authenticated: enters runs (and relay_used when relay)
    bool relay;
};
// h: the packet's first 16 bytes, read only when its length is 16 or more.
NEB_REPORT_HD inline ReportPacket report_packet(int32_t status, uint32_t raw_len, uint32_t key_id, const uint8_t* h,
                                                bool relayed) {
    ReportPacket r{};
    r.len = raw_len & ~NEB_RX_OWN_SOURCE;
    const ReportHeader hd = report_header(h, r.len);
    r.invalid = status == NEB_STATUS_INVALID && r.len > 1u;  // hole punches and padding are not counted
    r.rx_slot = report_past_gates(hd, raw_len, relayed) && hd.type != 1u ? report_rx_slot(hd.type, hd.sub) : kReportNoSlot;
    r.auth = status == NEB_STATUS_OK;
    r.relay = r.auth && hd.has && hd.type == 1u && hd.sub == 1u;
    r.relay_index = hd.index;
    const bool no_tunnel = status == NEB_STATUS_BAD_KEY && key_id == NEB_KEYS_MIXED;
    r.status_slot = r.auth                               ? NEB_METRIC_OPENED
                    : status == NEB_STATUS_AUTH_FAILED   ? NEB_METRIC_AUTH_FAILED
                    : status == NEB_STATUS_REPLAY        ? NEB_METRIC_REPLAY
                    : no_tunnel                          ? NEB_METRIC_NO_TUNNEL
                                                         : kReportNoSlot;
    if (hd.has) {
        if (status == NEB_STATUS_NOT_MESSAGE) {
            r.work = hd.type == 0u                                  ? NEB_WORK_HANDSHAKE
                     : hd.type == 2u                                ? NEB_WORK_RECV_ERROR
                     : relayed && hd.type == 1u && hd.sub == 1u     ? NEB_WORK_NESTED_RELAY
                                                                    : 0u;
        } else if (no_tunnel) {
            r.work = relayed ? 0u : NEB_WORK_SEND_RECV_ERROR;  // outside.go:105: not for a relayed packet
        } else if (r.auth) {
            r.work = hd.type == 3u                    ? NEB_WORK_LIGHTHOUSE
                     : hd.type == 4u && hd.sub == 0u  ? NEB_WORK_TEST_REQUEST
                     : hd.type == 5u                  ? NEB_WORK_CLOSE_TUNNEL
                     : hd.type == 6u                  ? NEB_WORK_CONTROL
                                                      : 0u;
        }
    }
    return r;
}

// A source as five words (a neb_udp_addr is compared as its 20 bytes).
struct ReportFrom {
    uint32_t w[5];
};
NEB_REPORT_HD inline bool report_same_from(const ReportFrom& a, const ReportFrom& b) {
    return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3] && a.w[4] == b.w[4];
}
// The index into from[] of packet i, or NEB_RECV_NONE: no source. Padding slots of the receive
// plan (pkt_entry = NEB_RECV_NONE) and entries past nfrom never index from[].
NEB_REPORT_HD inline uint32_t report_from_index(const void* from, const uint32_t* pkt_entry, uint32_t nfrom, uint32_t i,
                                                bool relayed) {
    if (!from || relayed) return NEB_RECV_NONE;
    const uint32_t j = pkt_entry ? pkt_entry[i] : i;
    return j == NEB_RECV_NONE || j >= nfrom ? NEB_RECV_NONE : j;
}
NEB_REPORT_HD inline ReportFrom report_from(const neb_udp_addr* from, const uint32_t* pkt_entry, uint32_t nfrom, uint32_t i,
                                            bool relayed) {
    ReportFrom f{};
    const uint32_t j = report_from_index(from, pkt_entry, nfrom, i, relayed);
    if (j != NEB_RECV_NONE) memcpy(f.w, __builtin_assume_aligned(&from[j], 4), sizeof f.w);
    return f;
}

// A run record as ten words behind its 8-byte-aligned start.
NEB_REPORT_HD inline void report_put_run(neb_rx_run* dst, uint64_t bytes, uint32_t key_id, uint32_t packet, uint32_t packets,
                                         const ReportFrom& f) {
    const uint32_t w[10] = {(uint32_t)bytes, (uint32_t)(bytes >> 32), key_id, packet, packets, f.w[0], f.w[1], f.w[2], f.w[3],
                            f.w[4]};
    memcpy(__builtin_assume_aligned(dst, 8), w, sizeof w);
}

}  // namespace neb
