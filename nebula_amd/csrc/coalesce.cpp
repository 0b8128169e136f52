// coalesce.cpp — neb_rx_coalesce_batch_host / neb_rx_plain_from_wire_host: MultiCoalescer.Flush as
// the reference runs it, packet by packet in sorted order, over the rules of coalesce_core.hpp. No
// HIP call: works without a GPU, and is what a single routine's 64-packet flush should use. The
// device form (coalesce.hip) computes the same result in parallel.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "coalesce_core.hpp"

namespace {

using namespace neb;

struct Slot {
    bool verbatim;
    uint32_t first;  // verbatim: the packet
    CoChain c;
    uint32_t tail;  // last member (chain order is kept in `next`)
};

// TCPCoalescer / UDPCoalescer: slots in creation order, one open chain per flow key.
struct Lane {
    bool tcp;
    std::vector<Slot> slots;
    std::unordered_map<std::string, uint32_t> open;  // flow key -> slot

    void add_verbatim(uint32_t i) { slots.push_back(Slot{true, i, CoChain{}, i}); }
};

inline bool span_ok(uint64_t off, uint64_t len, uint64_t total) { return off <= total && len <= total - off; }

}  // namespace

extern "C" NEB_API int neb_rx_coalesce_batch_host(const neb_plain_packet* plain, uint32_t n, const uint8_t* in,
                                                  size_t in_len, uint8_t* out, size_t out_cap, neb_tun_write* writes,
                                                  uint32_t max_writes, uint32_t* nwrites, uint32_t* pkt_write,
                                                  int32_t* pkt_status, uint32_t lanes) {
    if (!nwrites || (n && (!plain || !pkt_write || !pkt_status)) || (max_writes && !writes) || (out_cap && !out) ||
        (lanes & ~(uint32_t)(NEB_COALESCE_TCP | NEB_COALESCE_UDP)))
        return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (plain[i].flags & NEB_PLAIN_SKIP) continue;
        if (!span_ok(plain[i].off, plain[i].len, in_len) || (plain[i].len && !in)) return NEB_ERR_INVALID;
    }
    *nwrites = 0;

    // Commit: the class of every packet; Flush: the sort
    std::vector<CoRec> rec(n);
    std::vector<uint32_t> order;
    order.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        co_classify(plain[i], (plain[i].flags & NEB_PLAIN_SKIP) ? nullptr : in + plain[i].off, lanes, &rec[i]);
        pkt_status[i] = rec[i].status;
        pkt_write[i] = NEB_WRITE_NONE;
        if (rec[i].status == NEB_STATUS_OK) order.push_back(i);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (plain[a].epoch != plain[b].epoch) return plain[a].epoch < plain[b].epoch;
        return plain[a].counter < plain[b].counter;
    });

    // dispatch in transmission order
    Lane lane[2];
    lane[0].tcp = true;
    lane[1].tcp = false;
    std::vector<uint32_t> pt;
    std::vector<uint32_t> next(n, kCoNone);  // chain order
    uint8_t key[kCoKeyLen];
    for (uint32_t i : order) {
        const CoRec& r = rec[i];
        if (r.lane == kCoLanePt) {
            pt.push_back(i);
            continue;
        }
        Lane& L = lane[r.lane];
        const uint8_t* p = in + plain[i].off;
        if (r.cls == kCoUnparse) {  // sealAllOpen
            L.open.clear();
            L.add_verbatim(i);
            continue;
        }
        if (r.cls == kCoAck) {
            L.add_verbatim(i);
            continue;
        }
        co_flow_key(p, r.info, key);
        const std::string k((const char*)key, kCoKeyLen);
        if (r.cls == kCoSeal) {  // sealFlow
            L.open.erase(k);
            L.add_verbatim(i);
            continue;
        }
        auto it = L.open.find(k);
        if (it != L.open.end()) {
            Slot& s = L.slots[it->second];
            if (co_can_append(s.c, in + plain[s.c.first].off, p, r.info, L.tcp)) {
                next[s.tail] = i;
                s.tail = i;
                if (co_append(&s.c, r.info, L.tcp)) L.open.erase(it);
                continue;
            }
            L.open.erase(it);
        }
        Slot s{false, i, CoChain{}, i};
        co_seed(&s.c, i, r.info);
        L.slots.push_back(s);
        if (!(L.tcp && (r.info.flags & kCoTcpPsh))) L.open[k] = (uint32_t)L.slots.size() - 1;
    }

    // the lanes' Flush, in order, while the writes fit
    uint64_t off = 0;
    uint32_t w = 0;
    bool full = false;
    auto emit = [&](const Slot* s, uint32_t i, uint8_t ln) {
        const bool chain = s && !s->verbatim && s->c.nseg >= 2;
        const uint32_t len = chain ? s->c.hdr_len + s->c.total_pay : plain[i].len;
        if (!full && (w >= max_writes || off + co_align16(len) > out_cap)) full = true;
        if (full) {
            for (uint32_t m = i; m != kCoNone; m = chain ? next[m] : kCoNone) pkt_status[m] = NEB_STATUS_NO_SPACE;
            return;
        }
        uint8_t* o = out + off;
        if (!chain) {
            std::memcpy(o, in + plain[i].off, len);
            co_write_verbatim(&writes[w], off, len, i, ln);
            pkt_write[i] = w;
        } else {
            const CoChain& c = s->c;
            const bool tcp = ln == kCoLaneTcp;
            std::memcpy(o, in + plain[i].off, c.hdr_len);
            co_patch_header(o, c.v6, c.ip_hdr_len, c.hdr_len, c.total_pay, tcp, c.psh);
            uint32_t at = c.hdr_len;
            for (uint32_t m = i; m != kCoNone; m = next[m]) {
                std::memcpy(o + at, in + plain[m].off + rec[m].info.hdr_len, rec[m].info.pay_len);
                at += rec[m].info.pay_len;
                pkt_write[m] = w;
            }
            co_write_chain(&writes[w], off, i, c.nseg, c.hdr_len, c.ip_hdr_len, c.total_pay, c.gso, c.v6, tcp);
        }
        off += co_align16(len);
        w++;
    };
    for (int l = 0; l < 2; l++)
        for (const Slot& s : lane[l].slots) emit(&s, s.first, (uint8_t)l);
    for (uint32_t i : pt) emit(nullptr, i, kCoLanePt);
    *nwrites = w;
    return NEB_OK;
}

extern "C" NEB_API int neb_rx_plain_from_wire_host(const neb_rx_packet* pk, const int32_t* status,
                                                   const uint64_t* epoch, uint32_t nepoch, uint32_t n,
                                                   const uint8_t* arena, size_t arena_len, neb_plain_packet* plain) {
    if ((n && (!pk || !status || !plain || !arena)) || (nepoch && !epoch)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if (!span_ok(pk[i].off, pk[i].len & ~NEB_RX_OWN_SOURCE, arena_len)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) co_plain_from_wire(pk[i], status[i], arena, epoch, nepoch, &plain[i]);
    return NEB_OK;
}
