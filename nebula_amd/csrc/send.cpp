// send.cpp — neb_tx_send_plan_host: WriteBatch's packing loop as the reference runs it, run by run in
// wire order, over the rules of send_core.hpp. No HIP call: works without a GPU. The device form
// (send.hip) computes the same plan in parallel.
#include "send_core.hpp"

using namespace neb;

extern "C" NEB_API int neb_tx_send_plan_host(const neb_tx_wire* wires, const int32_t* wire_status, uint32_t nwires,
                                             const neb_tx_packet* packets, uint32_t npackets,
                                             const neb_relay_route* via, const neb_udp_addr* remote,
                                             uint32_t ntunnels, uint32_t socket_v4, uint32_t max_segments,
                                             uint32_t chunk_packets, neb_send_iov* iov, uint32_t* niov,
                                             neb_send_entry* entries, uint32_t* nentries, uint32_t* wire_entry,
                                             int32_t* send_status) {
    if (max_segments > kSendMaxSegments || !niov || !nentries || (npackets && !packets) || (ntunnels && !remote) ||
        (nwires && (!wires || !wire_status || !iov || !entries || !wire_entry || !send_status)))
        return NEB_ERR_INVALID;
    const uint32_t ms = send_max_segments(max_segments);
    uint32_t ni = 0, ne = 0;
    // the run being planned: entries[ne], open while a next packet may still join it
    bool open = false;
    SendRec head{};
    uint32_t run_max = 0;
    for (uint32_t i = 0; i < nwires; i++) {
        SendRec r;
        send_classify(wires[i], wire_status[i], packets, npackets, via, remote, ntunnels, socket_v4, &r);
        send_status[i] = send_status_of(r.cls);
        wire_entry[i] = NEB_SEND_NONE;
        if (r.cls == kSendAbsent) continue;  // not among the bufs
        if (r.cls != kSendRoutable) {        // a skipped run: no iovec, but the run before it has ended
            open = false;
            continue;
        }
        neb_send_entry* en = open ? &entries[ne - 1] : nullptr;
        const bool joins = en && en->niov < run_max && r.len != 0u && r.len <= head.len && send_same_dst(head, r) &&
                           en->bytes + r.len <= NEB_SEND_MAX_BYTES;
        if (joins) {
            en->niov++;
            en->bytes += r.len;
            en->seg_size = (uint16_t)head.len;
            if (r.len < head.len) open = false;  // a short packet is the last of its run
        } else {
            // planRun at this packet: the iovec budget is what is left of the chunk
            const uint32_t budget = chunk_packets ? chunk_packets - ni % chunk_packets : ms;
            run_max = budget < ms ? budget : ms;
            head = r;
            entries[ne] = neb_send_entry{ni, 1, 0, r.dst, r.len};
            ne++;
            open = r.len != 0u && r.len <= NEB_SEND_MAX_BYTES;
        }
        iov[ni] = neb_send_iov{wires[i].out_off, r.len, i};
        wire_entry[i] = ne - 1;
        ni++;
    }
    *niov = ni;
    *nentries = ne;
    return NEB_OK;
}
