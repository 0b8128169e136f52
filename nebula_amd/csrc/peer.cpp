// peer.cpp — neb_peer_table_* and neb_rx_inner_batch[_host]: the table of every tunnel's certificate
// networks (HostInfo.networks) and the node's routable set (rules: peer_core.hpp). The host copy is
// authoritative, as in route.cpp: every update is applied to it first under the table's lock, and
// neb_rx_inner_batch_host reads it. A table made with an engine also keeps a device copy
// (table_mirror.hpp), written by route.hip's scatter: the slots are the TX table's. Compiled
// without HIP (g++: tests/sanitize_peer) only the host-only table exists.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "host_common.hpp"  // span_in
#include "peer_core.hpp"
#include "table_mirror.hpp"

#if defined(__HIPCC__)
#include "engine_internal.hpp"
#include "hip_guard.hpp"
#include "peer.hpp"
#include "route.hpp"  // TxOp, neb_txt_scatter
#endif

using namespace neb;

namespace {

constexpr uint32_t kPeerMaxCapacity = 1u << 20;
using PeerKey = std::tuple<uint32_t, uint32_t, uint32_t, uint64_t, uint64_t>;  // tunnel, family, bits, hi, lo (masked)
struct PeerTouch {  // one key an update names
    bool live;      // is it live now
    int32_t fresh;  // the slot this call filled for it, as an index into `fresh`, or -1
};

inline PeerKey peer_key(uint32_t tunnel, const neb_cidr& c) {
    const TxAddr a = tx_addr_from_bytes(c.addr, c.family), m = tx_prefix_mask(c.bits);
    return PeerKey{tunnel, c.family, c.bits, a.hi & m.hi, a.lo & m.lo};
}
inline TxAddr peer_addr(const PeerKey& k) { return TxAddr{std::get<3>(k), std::get<4>(k)}; }

}  // namespace

struct neb_peer_table {
    uint32_t cap = 0, mask = 0;
    // mu: the host copy, the routable set and, for writers, the order of the updates' device work
    mutable std::shared_mutex mu;
    std::vector<TxSlot> slots;
    uint32_t used = 0;  // live + tombstones
    std::map<PeerKey, uint32_t> nets;  // -> NEB_NET_*
    uint32_t count4[33] = {}, count6[129] = {};  // live entries per prefix length
    TxLens lens{};
    PeerRoutable routable{};
#if defined(__HIPCC__)
    int device = -1;  // -1: host-only
    // the device copy; its lock (also dlens' and droutable's) is taken inside mu by writers, alone by
    // neb_rx_inner_batch
    TableMirror<HipWsApi, TxSlot, TxOp> dev;
    TxLens dlens{};  // a superset of the lengths in the image a launch will read
    PeerRoutable droutable{};
#endif
};

namespace {

inline bool peer_find_host(const neb_peer_table* t, const PeerKey& k, uint32_t* slot, uint32_t* probes) {
    return peer_find(t->slots.data(), t->mask, std::get<0>(k), std::get<1>(k), std::get<2>(k), peer_addr(k), HostLoad{}, slot,
                     probes);
}

// Puts a record into the first EMPTY slot of its chain (the table always has one).
uint32_t peer_insert(neb_peer_table* t, const PeerKey& k, uint32_t type) {
    const TxAddr a = peer_addr(k);
    const uint64_t h = peer_hash(std::get<0>(k), std::get<1>(k), std::get<2>(k), a);
    uint32_t s = (uint32_t)h & t->mask;
    while (t->slots[s].tag != kTxEmpty) s = (s + 1u) & t->mask;
    t->slots[s] = TxSlot{peer_tag(std::get<0>(k), std::get<1>(k), std::get<2>(k), h), a.lo, a.hi, type};
    t->used++;
    return s;
}

void peer_rebuild_slots(neb_peer_table* t) {  // no tombstones
    std::fill(t->slots.begin(), t->slots.end(), TxSlot{});
    t->used = 0;
    for (const auto& n : t->nets) peer_insert(t, n.first, n.second);
}

void peer_count(neb_peer_table* t, const PeerKey& k, int by) {
    uint32_t* c = std::get<1>(k) == 4 ? &t->count4[std::get<2>(k)] : &t->count6[std::get<2>(k)];
    *c = (uint32_t)((int64_t)*c + by);
}
void peer_set_lens(neb_peer_table* t) {
    t->lens = TxLens{};
    for (uint32_t b = 0; b <= 32; b++)
        if (t->count4[b]) tx_lens_add(&t->lens, 4, b);
    for (uint32_t b = 0; b <= 128; b++)
        if (t->count6[b]) tx_lens_add(&t->lens, 6, b);
}

#if defined(__HIPCC__)
void peer_delete_device(neb_peer_table* t) {
    DeviceGuard dg(t->device);
    t->dev.drain();
    delete t;
}
#endif

}  // namespace

extern "C" NEB_API int neb_peer_table_create(neb_engine* e, uint32_t capacity, neb_peer_table** out) {
    if (!out || capacity == 0 || capacity > kPeerMaxCapacity) return NEB_ERR_INVALID;
    *out = nullptr;
#if !defined(__HIPCC__)
    if (e) return NEB_ERR_NO_DEVICE;
#endif
    neb_peer_table* t = new (std::nothrow) neb_peer_table;
    if (!t) return NEB_ERR_INVALID;
    t->cap = capacity;
    try {
        t->slots.assign(tx_slots_for(capacity), TxSlot{});
    } catch (const std::bad_alloc&) {
        delete t;
        return NEB_ERR_INVALID;
    }
    t->mask = (uint32_t)t->slots.size() - 1u;
#if defined(__HIPCC__)
    if (e) {
        t->device = neb_engine_device_of(e);
        DeviceGuard dg(t->device);
        const int rc = t->dev.init(t->slots.size());
        if (rc != NEB_OK) {
            peer_delete_device(t);
            return rc;
        }
    }
#endif
    *out = t;
    return NEB_OK;
}

extern "C" NEB_API int neb_peer_table_destroy(neb_peer_table* t) {
    if (!t) return NEB_ERR_INVALID;
#if defined(__HIPCC__)
    if (t->device >= 0) {
        peer_delete_device(t);
        return NEB_OK;
    }
#endif
    delete t;
    return NEB_OK;
}

extern "C" NEB_API int neb_peer_table_update(neb_peer_table* t, const neb_peer_key* del, uint32_t ndel,
                                             const neb_peer_net* put, uint32_t nput, void* stream) try {
    if (!t || (ndel && !del) || (nput && !put)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < ndel; i++)
        if (!cidr_ok(del[i].prefix) || del[i].tunnel == NEB_KEYS_MIXED) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < nput; i++)
        if (!cidr_ok(put[i].prefix) || put[i].tunnel == NEB_KEYS_MIXED || put[i].type < NEB_NET_VPN || put[i].type > NEB_NET_UNSAFE)
            return NEB_ERR_INVALID;
    std::unique_lock<std::shared_mutex> g(t->mu);
    // Everything that allocates comes first, so that an allocation failure applies nothing.
    // Entries live after the call: the deletions, then the puts, over the keys the call names.
    std::map<PeerKey, PeerTouch> now;
    int64_t live = (int64_t)t->nets.size();
    auto touch = [&](const PeerKey& k, bool to) {
        auto it = now.find(k);
        if (it == now.end()) it = now.emplace(k, PeerTouch{t->nets.count(k) != 0, -1}).first;
        live += (int)to - (int)it->second.live;
        it->second.live = to;
    };
    for (uint32_t i = 0; i < ndel; i++) touch(peer_key(del[i].tunnel, del[i].prefix), false);
    for (uint32_t i = 0; i < nput; i++) touch(peer_key(put[i].tunnel, put[i].prefix), true);
    if (live > (int64_t)t->cap) return NEB_ERR_NO_KEY_SLOT;
    std::map<PeerKey, uint32_t> add;  // the puts' last word per key, as nodes ready to move into nets
    for (uint32_t i = 0; i < nput; i++) add[peer_key(put[i].tunnel, put[i].prefix)] = put[i].type;
    // every put takes a slot; past 3/4 of the slots in use the table is rebuilt without its tombstones
    const bool rebuild = (uint64_t)t->used + nput > (uint64_t)(t->mask + 1u) / 4u * 3u;
    std::vector<std::pair<uint32_t, bool>> fresh;  // the slots filled, and whether each is live at the end
    std::vector<uint32_t> dead;                    // the slots live before the call that it tombstoned
    if (!rebuild) {
        fresh.reserve(nput);
        dead.reserve((size_t)ndel + nput);
    }
#if defined(__HIPCC__)
    std::vector<TxOp> first, second;
    if (!rebuild && t->device >= 0) {
        first.reserve(nput);
        second.reserve((size_t)ndel + nput);
    }
#endif
    // From here on nothing allocates on the host.
    if (!rebuild) {
        auto bury = [&](uint32_t s, PeerTouch* tc) {
            t->slots[s].tag = kTxTomb;
            if (tc->fresh >= 0) fresh[(size_t)tc->fresh].second = false;
            else dead.push_back(s);
            tc->fresh = -1;
        };
        uint32_t s, p;
        for (uint32_t i = 0; i < ndel; i++) {
            const PeerKey k = peer_key(del[i].tunnel, del[i].prefix);
            if (peer_find_host(t, k, &s, &p)) bury(s, &now.find(k)->second);
        }
        for (uint32_t i = 0; i < nput; i++) {
            const PeerKey k = peer_key(put[i].tunnel, put[i].prefix);
            PeerTouch* tc = &now.find(k)->second;
            const bool had = peer_find_host(t, k, &s, &p);
            fresh.emplace_back(peer_insert(t, k, put[i].type), true);  // behind the old record
            if (had) bury(s, tc);
            tc->fresh = (int32_t)fresh.size() - 1;
        }
    }
    for (uint32_t i = 0; i < ndel; i++) {
        const PeerKey k = peer_key(del[i].tunnel, del[i].prefix);
        if (t->nets.erase(k)) peer_count(t, k, -1);
    }
    while (!add.empty()) {
        auto node = add.extract(add.begin());
        auto it = t->nets.find(node.key());
        if (it != t->nets.end()) {
            it->second = node.mapped();
        } else {
            peer_count(t, node.key(), 1);
            t->nets.insert(std::move(node));
        }
    }
    peer_set_lens(t);
    if (rebuild) peer_rebuild_slots(t);
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        if (rebuild)
            return t->dev.rebuild(t->slots.data(), (hipStream_t)stream, [](int, hipStream_t) { return hipSuccess; },
                                  [&](int) { t->dlens = t->lens; });
        {
            // before the scatter, so a launch that can see a new record also probes its length. A launch
            // on another stream that gets these lengths but still reads the old records can only miss
            // an entry of a length this call emptied: an entry this call deletes.
            std::lock_guard<std::mutex> dl(t->dev.lock());
            t->dlens = t->lens;
        }
        for (const auto& f : fresh) {
            const TxSlot& sl = t->slots[f.first];
            first.push_back(f.second ? TxOp{f.first, sl.tag, sl.addr_lo, sl.addr_hi, sl.value} : TxOp{f.first, kTxTomb, 0, 0, 0});
        }
        for (uint32_t d : dead) second.push_back(TxOp{d, kTxTomb, 0, 0, 0});
        return t->dev.update(first, second, (hipStream_t)stream, [&](TxSlot* image, const TxOp* ops, uint32_t cnt, hipStream_t s) {
            return neb_txt_scatter(image, t->mask, ops, cnt, s);
        });
    }
#endif
    (void)stream;
    return NEB_OK;
} catch (const std::bad_alloc&) {
    return NEB_ERR_INVALID;
}

extern "C" NEB_API int neb_peer_table_set_routable(neb_peer_table* t, const neb_cidr* nets, uint32_t n) {
    if (!t || n > NEB_RX_MAX_ROUTABLE || (n && !nets)) return NEB_ERR_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!cidr_ok(nets[k])) return NEB_ERR_INVALID;
    PeerRoutable v;
    peer_routable_set(&v, nets, n);
    std::unique_lock<std::shared_mutex> g(t->mu);
    t->routable = v;
#if defined(__HIPCC__)
    std::lock_guard<std::mutex> dg(t->dev.lock());
    t->droutable = v;
#endif
    return NEB_OK;
}

extern "C" NEB_API int neb_peer_table_count(const neb_peer_table* t, uint32_t* live) {
    if (!t || !live) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    *live = (uint32_t)t->nets.size();
    return NEB_OK;
}

extern "C" NEB_API int neb_peer_table_probe(const neb_peer_table* t, const neb_peer_key* key, uint32_t out[3]) {
    if (!t || !key || !out || !cidr_ok(key->prefix)) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    out[0] = peer_find_host(t, peer_key(key->tunnel, key->prefix), &out[1], &out[2]);
    return NEB_OK;
}

extern "C" NEB_API int neb_rx_inner_batch_host(const neb_peer_table* t, const neb_rx_packet* pk, const int32_t* status,
                                               const uint64_t* epoch, uint32_t nepoch, uint32_t n, const uint8_t* arena,
                                               size_t arena_len, neb_plain_packet* plain, neb_fw_packet* fw,
                                               int32_t* inner_status) {
    if (!t || (n && (!pk || !status || !plain || !arena)) || (nepoch && !epoch)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if (!span_in(pk[i].off, pk[i].len & ~NEB_RX_OWN_SOURCE, arena_len)) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* h = arena + pk[i].off;
        auto hdr = [&](uint32_t k) -> uint32_t { return h[k]; };
        auto body = [&](uint32_t k) -> uint32_t { return h[16u + k]; };
        auto ep = [&](uint32_t k) { return epoch[k]; };
        auto look = [&](uint32_t family, uint32_t bits, const TxAddr& a, uint64_t* v) {
            uint32_t s, probes;
            if (!peer_find(t->slots.data(), t->mask, pk[i].key_id, family, bits, a, HostLoad{}, &s, &probes)) return false;
            *v = t->slots[s].value;
            return true;
        };
        PeerResult r;
        peer_inner_one(pk[i].off, pk[i].len & ~NEB_RX_OWN_SOURCE, pk[i].key_id, status[i], nepoch, hdr, body, ep, t->lens,
                       t->routable, look, &r);
        std::memcpy(&plain[i], r.plain, sizeof(neb_plain_packet));
        if (fw) std::memcpy(&fw[i], r.fw, sizeof(neb_fw_packet));
        if (inner_status) inner_status[i] = r.status;
    }
    return NEB_OK;
}

extern "C" NEB_API int neb_rx_inner_batch(neb_engine* e, const neb_peer_table* t, const neb_rx_packet* d_pk,
                                          const int32_t* d_status, const uint64_t* d_epoch, uint32_t nepoch, uint32_t n,
                                          const uint8_t* d_arena, neb_plain_packet* d_plain, neb_fw_packet* d_fw,
                                          int32_t* d_inner_status, void* stream) {
#if defined(__HIPCC__)
    if (!e || !t || t->device < 0 || t->device != neb_engine_device_of(e) ||
        (n && (!d_pk || !d_status || !d_arena || !d_plain)) || (nepoch && !d_epoch) ||
        ((reinterpret_cast<uintptr_t>(d_plain) | reinterpret_cast<uintptr_t>(d_fw)) & 15u))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    // the mirror's lock only: a compaction in progress holds mu and does not stall this call
    DeviceGuard dg(t->device);
    return t->dev.read((hipStream_t)stream, [&](int, const TxSlot* image) {
        return neb_peer_inner(image, t->mask, &t->dlens, &t->droutable, d_pk, d_status, d_epoch, nepoch, n, d_arena, d_plain,
                              d_fw, d_inner_status, (hipStream_t)stream);
    });
#else
    (void)e, (void)t, (void)d_pk, (void)d_status, (void)d_epoch, (void)nepoch, (void)n, (void)d_arena, (void)d_plain, (void)d_fw,
        (void)d_inner_status, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}
