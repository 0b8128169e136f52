// recv.cpp — neb_rx_recv_plan_host: ListenOut's loop over a recvmmsg batch as the reference runs it,
// entry by entry, over the rules of recv_core.hpp. No HIP call: works without a GPU. The device form
// (recv.hip) computes the same plan in parallel.
#include "recv_core.hpp"

using namespace neb;

namespace {
// The ABI aligns the outputs to 4 bytes only.
void put_pk(neb_rx_packet* pk, uint64_t off, uint32_t len) {
    const neb_rx_packet v{off, len, NEB_KEYS_MIXED};
    memcpy(pk, &v, sizeof v);
}
void put_words(void* dst, const RecvFrom& f, uint32_t last) {
    const uint32_t w[5] = {f.a[0], f.a[1], f.a[2], f.a[3], last};
    memcpy(dst, w, sizeof w);
}
}  // namespace

extern "C" NEB_API int neb_rx_recv_plan_host(const neb_recv_entry* entries, uint32_t nentries, const uint8_t* ctrl,
                                             uint32_t ctrl_stride, uint32_t socket_v4, neb_rx_packet* pk,
                                             neb_rx_source* src, uint32_t* pkt_entry, uint32_t max_packets,
                                             neb_udp_addr* from, uint32_t* entry_first, uint32_t* counts) {
    if (!pk || !entry_first || !counts || (nentries && !entries) || nentries > 0x7FFFFFFFu || max_packets > 0x7FFFFFFFu ||
        (ctrl && (ctrl_stride == 0u || (ctrl_stride & 7u) || ctrl_stride > kRecvMaxCtrlStride)))
        return NEB_ERR_INVALID;
    uint32_t np = 0, done = 0;
    bool cut = false;  // the emitted entries are a prefix
    for (uint32_t j = 0; j < nentries; j++) {
        const neb_recv_entry& en = entries[j];
        uint32_t name[7];
        memcpy(name, en.name, sizeof name);
        const RecvFrom f = recv_from(name, socket_v4);
        if (from) put_words(&from[j], f, recv_addr_word(f));
        entry_first[j] = NEB_RECV_NONE;
        if (cut) continue;
        const int32_t seg = recv_seg_size(en, ctrl, ctrl_stride, j);
        const uint64_t cnt = recv_count(en.len, seg);
        if (!recv_emitted(np, cnt, max_packets)) {
            cut = true;
            continue;
        }
        entry_first[j] = np;
        for (uint64_t k = 0; k < cnt; k++, np++) {
            uint64_t off;
            uint32_t len;
            recv_packet(en.off, en.len, seg, k, &off, &len);
            put_pk(&pk[np], off, len);
            if (src) put_words(&src[np], f, recv_source_word(f));
            if (pkt_entry) pkt_entry[np] = j;
        }
        done = j + 1u;
    }
    for (uint32_t i = np; i < max_packets; i++) {  // padding: the receive calls' gate refuses it
        put_pk(&pk[i], 0, 0);
        if (src) memset(&src[i], 0, sizeof(neb_rx_source));
        if (pkt_entry) pkt_entry[i] = NEB_RECV_NONE;
    }
    counts[0] = np;
    counts[1] = done;
    return NEB_OK;
}
