// report.cpp — neb_rx_report_batch_host: the RX batch report as one sequential pass over the packets
// and one sort of the authenticated ones, over the rules of report_core.hpp. No HIP call: works
// without a GPU. The device form (report.hip) computes the same report in parallel.
#include <algorithm>
#include <vector>

#include "report_core.hpp"

using namespace neb;

namespace {
struct Auth {
    uint32_t key_id, packet, len;
};
// The ABI aligns the records to 4 bytes only.
void put2(void* dst, uint32_t a, uint32_t b) {
    const uint32_t w[2] = {a, b};
    memcpy(dst, w, sizeof w);
}
neb_rx_packet get_pk(const neb_rx_packet* pk, uint32_t i) {
    neb_rx_packet p;
    memcpy(&p, &pk[i], sizeof p);
    return p;
}
}  // namespace

extern "C" NEB_API int neb_rx_report_batch_host(const neb_rx_packet* pk, const int32_t* status, uint32_t n, const uint8_t* arena,
                                                size_t arena_len, const neb_udp_addr* from, const uint32_t* pkt_entry,
                                                uint32_t nfrom, uint32_t flags, neb_rx_run* runs, neb_rx_relay_used* relay_used,
                                                neb_rx_work* work, uint64_t* metrics, uint32_t* counts) {
    if (!metrics || !counts || n > 0x7FFFFFFFu || (flags & ~NEB_REPORT_RELAYED) ||
        (n && (!pk || !status || !arena || !runs || !relay_used || !work)) || (reinterpret_cast<uintptr_t>(runs) & 7u) ||
        (reinterpret_cast<uintptr_t>(metrics) & 7u) ||
        ((reinterpret_cast<uintptr_t>(pk) | reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(from) |
          reinterpret_cast<uintptr_t>(pkt_entry) | reinterpret_cast<uintptr_t>(relay_used) | reinterpret_cast<uintptr_t>(work) |
          reinterpret_cast<uintptr_t>(counts)) &
         3u))
        return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {  // before anything is written
        const neb_rx_packet p = get_pk(pk, i);
        const uint32_t len = p.len & ~NEB_RX_OWN_SOURCE;
        if (len >= 16u && (p.off > arena_len || len > arena_len - p.off)) return NEB_ERR_INVALID;
    }
    const bool relayed = flags & NEB_REPORT_RELAYED;
    uint64_t m[kReportMetrics] = {};
    uint32_t nwork = 0;
    std::vector<Auth> auth;
    std::vector<uint32_t> relay;
    for (uint32_t i = 0; i < n; i++) {
        const neb_rx_packet p = get_pk(pk, i);
        const uint8_t* h = (p.len & ~NEB_RX_OWN_SOURCE) >= 16u ? arena + p.off : arena;  // off is checked only then
        const ReportPacket r = report_packet(status[i], p.len, p.key_id, h, relayed);
        m[NEB_METRIC_RX_INVALID] += r.invalid;
        if (r.rx_slot != kReportNoSlot) m[r.rx_slot]++;
        if (r.status_slot != kReportNoSlot) m[r.status_slot]++;
        if (r.work) put2(&work[nwork++], i, r.work);
        if (r.auth) {
            m[NEB_METRIC_OPENED_BYTES] += r.len;
            auth.push_back({p.key_id, i, r.len});
            if (r.relay) relay.push_back(r.relay_index);
        }
    }
    // by (key_id, packet index): the packets arrive in index order, so a stable sort by key_id
    std::stable_sort(auth.begin(), auth.end(), [](const Auth& a, const Auth& b) { return a.key_id < b.key_id; });
    uint32_t nruns = 0, ntunnels = 0, packets = 0, first = 0, key = 0;
    uint64_t bytes = 0;
    ReportFrom cur{};
    for (size_t k = 0; k < auth.size(); k++) {
        const Auth& a = auth[k];
        const ReportFrom f = report_from(from, pkt_entry, nfrom, a.packet, relayed);
        const bool tunnel_head = k == 0 || a.key_id != key;
        if (tunnel_head || !report_same_from(f, cur)) {
            if (k) report_put_run(&runs[nruns++], bytes, key, first, packets, cur);
            ntunnels += tunnel_head;
            key = a.key_id, first = a.packet, cur = f, packets = 0, bytes = 0;
        }
        packets++;
        bytes += a.len;
    }
    if (!auth.empty()) report_put_run(&runs[nruns++], bytes, key, first, packets, cur);
    std::sort(relay.begin(), relay.end());
    uint32_t nrelay = 0;
    for (size_t k = 0; k < relay.size();) {
        size_t e = k;
        while (e < relay.size() && relay[e] == relay[k]) e++;
        put2(&relay_used[nrelay++], relay[k], (uint32_t)(e - k));
        k = e;
    }
    memcpy(metrics, m, sizeof m);
    const uint32_t c[4] = {nruns, ntunnels, nrelay, nwork};
    memcpy(counts, c, sizeof c);
    return NEB_OK;
}
