// route.cpp — neb_tx_table_* and neb_tx_resolve_batch[_host]: the table of the TX-side lookups (VPN
// address -> tunnel, unsafe routes, ECMP gateways; rules: route_core.hpp). The host copy is
// authoritative: every update is applied to it first under the table's lock, and
// neb_tx_resolve_batch_host reads it. A table made with an engine also keeps a device copy
// (table_mirror.hpp), written by route.hip's scatter; each image has its gateway array and set of
// prefix lengths, so a compaction and every neb_tx_table_set_routes go through a rebuild. Compiled
// without HIP (g++: tests/sanitize_route) only the host-only table exists.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <shared_mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "route_core.hpp"
#include "table_mirror.hpp"

#if defined(__HIPCC__)
#include "engine_internal.hpp"
#include "hip_guard.hpp"
#include "route.hpp"
#endif

using namespace neb;

namespace {

constexpr uint32_t kTxMaxCapacity = 1u << 20;  // per kind: a host copy of at most 256 MiB
using TxKey = std::tuple<uint32_t, uint64_t, uint64_t>;  // family, hi, lo
struct TxTouch {  // one address an update names
    bool live;      // is it live now
    int32_t fresh;  // the slot this call filled for it, as an index into `fresh`, or -1
};
struct TxRouteRec {
    uint32_t family, bits;
    TxAddr addr;  // masked
    uint32_t first, count;
};

inline bool tx_family_ok(uint32_t f) { return f == 4 || f == 6; }
inline TxKey tx_key(const neb_tx_addr& a) {
    const TxAddr v = tx_addr_from_bytes(a.addr, a.family);
    return TxKey{a.family, v.hi, v.lo};
}

}  // namespace

struct neb_tx_table {
    uint32_t host_cap = 0, route_cap = 0, gw_cap = 0, mask = 0;
    // mu: the host copy, the own networks and, for writers, the order of the updates' device work
    mutable std::shared_mutex mu;
    std::vector<TxSlot> slots;
    uint32_t used = 0;  // live + tombstones
    std::map<TxKey, uint32_t> hosts;
    std::vector<TxRouteRec> routes;
    std::vector<TxGw> gws;
    TxLens lens{};
    TxOwn own{};
#if defined(__HIPCC__)
    int device = -1;  // -1: host-only
    // the device copy; its lock (also `down`'s) is taken inside mu by writers, alone by the resolve
    TableMirror<HipWsApi, TxSlot, TxOp> dev;
    DevBuf<TxGw> dgw[2];
    TxLens dlens[2] = {};  // switch with the image
    TxOwn down{};          // own, for the device resolve: it never takes mu
    PinnedBuf<TxGw> upload_gw;
#endif
};

namespace {

inline bool tx_find_host(const neb_tx_table* t, uint32_t kind, uint32_t family, uint32_t bits, const TxAddr& a,
                         uint32_t* slot, uint32_t* probes) {
    return tx_find(t->slots.data(), t->mask, kind, family, bits, a, HostLoad{}, slot, probes);
}

// Puts a record into the first EMPTY slot of its chain (the table always has one).
uint32_t tx_insert(neb_tx_table* t, uint32_t kind, uint32_t family, uint32_t bits, const TxAddr& a, uint64_t value) {
    const uint64_t h = tx_hash(kind, family, bits, a);
    uint32_t s = (uint32_t)h & t->mask;
    while (t->slots[s].tag != kTxEmpty) s = (s + 1u) & t->mask;
    t->slots[s] = TxSlot{tx_tag(kind, family, bits, h), a.lo, a.hi, value};
    t->used++;
    return s;
}

// The slots from the hosts and the routes: no tombstones.
void tx_rebuild_slots(neb_tx_table* t) {
    std::fill(t->slots.begin(), t->slots.end(), TxSlot{});
    t->used = 0;
    for (const auto& h : t->hosts)
        tx_insert(t, NEB_TX_KIND_HOST, std::get<0>(h.first), 0, TxAddr{std::get<1>(h.first), std::get<2>(h.first)}, h.second);
    for (const TxRouteRec& r : t->routes)
        tx_insert(t, NEB_TX_KIND_ROUTE, r.family, r.bits, r.addr, r.first | ((uint64_t)r.count << 32));
}

// The host update on the slots of the host copy, one by one. fresh: the slots it filled, and whether
// each is still live at the end; dead: the slots live before the call that it tombstoned. Allocates
// nothing: the caller has reserved fresh and dead, and `now` holds every address the call names.
void tx_apply(neb_tx_table* t, const neb_tx_addr* del, uint32_t ndel, const neb_tx_host* put, uint32_t nput,
              std::map<TxKey, TxTouch>* now, std::vector<std::pair<uint32_t, bool>>* fresh, std::vector<uint32_t>* dead) {
    auto bury = [&](uint32_t s, TxTouch* tc) {
        t->slots[s].tag = kTxTomb;
        if (tc->fresh >= 0) (*fresh)[(size_t)tc->fresh].second = false;
        else dead->push_back(s);
        tc->fresh = -1;
    };
    uint32_t s, p;
    for (uint32_t i = 0; i < ndel; i++) {
        const TxAddr a = tx_addr_from_bytes(del[i].addr, del[i].family);
        if (tx_find_host(t, NEB_TX_KIND_HOST, del[i].family, 0, a, &s, &p)) bury(s, &now->find(tx_key(del[i]))->second);
    }
    for (uint32_t i = 0; i < nput; i++) {
        const TxAddr a = tx_addr_from_bytes(put[i].addr.addr, put[i].addr.family);
        TxTouch* tc = &now->find(tx_key(put[i].addr))->second;
        const bool had = tx_find_host(t, NEB_TX_KIND_HOST, put[i].addr.family, 0, a, &s, &p);
        fresh->emplace_back(tx_insert(t, NEB_TX_KIND_HOST, put[i].addr.family, 0, a, put[i].tunnel), true);  // behind the old record
        if (had) bury(s, tc);
        tc->fresh = (int32_t)fresh->size() - 1;
    }
}

#if defined(__HIPCC__)
// The rebuilt host copy and the gateways into the spare image, then the switch of image, gateways
// and prefix lengths together (mu held exclusively). Blocks.
int tx_push_rebuild(neb_tx_table* t, hipStream_t s) {
    auto gateways = [&](int spare, hipStream_t st) {
        const size_t gbytes = t->gws.size() * sizeof(TxGw);
        if (!gbytes) return hipSuccess;
        std::memcpy(t->upload_gw, t->gws.data(), gbytes);
        return HipWsApi::copy_h2d(t->dgw[spare], t->upload_gw, gbytes, st);
    };
    return t->dev.rebuild(t->slots.data(), s, gateways, [&](int spare) { t->dlens[spare] = t->lens; });
}

// Waits for the device work on the table, then deletes it: its members release themselves, with
// the table's device current.
void tx_delete_device(neb_tx_table* t) {
    DeviceGuard dg(t->device);
    t->dev.drain();
    delete t;
}

int tx_init_device(neb_tx_table* t) {
    const size_t gbytes = std::max<size_t>(1, t->gw_cap) * sizeof(TxGw);
    for (int k = 0; k < 2; k++)
        if (t->dgw[k].reserve(gbytes) != hipSuccess || HipWsApi::memset(t->dgw[k], 0, gbytes) != hipSuccess) return NEB_ERR_HIP;
    if (t->upload_gw.reserve(gbytes) != hipSuccess) return NEB_ERR_HIP;
    return t->dev.init(t->slots.size());  // (synchronises the device: the gateway arrays are zero too)
}
#endif

}  // namespace

extern "C" NEB_API int neb_tx_table_create(neb_engine* e, uint32_t host_capacity, uint32_t route_capacity,
                                           uint32_t gateway_capacity, neb_tx_table** out) {
    if (!out || host_capacity == 0 || host_capacity > kTxMaxCapacity || route_capacity > kTxMaxCapacity ||
        gateway_capacity > kTxMaxCapacity)
        return NEB_ERR_INVALID;
    *out = nullptr;
#if !defined(__HIPCC__)
    if (e) return NEB_ERR_NO_DEVICE;
#endif
    neb_tx_table* t = new (std::nothrow) neb_tx_table;
    if (!t) return NEB_ERR_INVALID;
    t->host_cap = host_capacity;
    t->route_cap = route_capacity;
    t->gw_cap = gateway_capacity;
    try {
        t->slots.assign(tx_slots_for(host_capacity + route_capacity), TxSlot{});
    } catch (const std::bad_alloc&) {
        delete t;
        return NEB_ERR_INVALID;
    }
    t->mask = (uint32_t)t->slots.size() - 1u;
#if defined(__HIPCC__)
    if (e) {
        t->device = neb_engine_device_of(e);
        DeviceGuard dg(t->device);
        const int rc = tx_init_device(t);
        if (rc != NEB_OK) {
            tx_delete_device(t);
            return rc;
        }
    }
#endif
    *out = t;
    return NEB_OK;
}

extern "C" NEB_API int neb_tx_table_destroy(neb_tx_table* t) {
    if (!t) return NEB_ERR_INVALID;
#if defined(__HIPCC__)
    if (t->device >= 0) {
        tx_delete_device(t);
        return NEB_OK;
    }
#endif
    delete t;
    return NEB_OK;
}

extern "C" NEB_API int neb_tx_table_update_hosts(neb_tx_table* t, const neb_tx_addr* del, uint32_t ndel,
                                                 const neb_tx_host* put, uint32_t nput, void* stream) try {
    if (!t || (ndel && !del) || (nput && !put)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < ndel; i++)
        if (!tx_family_ok(del[i].family)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < nput; i++)
        if (!tx_family_ok(put[i].addr.family)) return NEB_ERR_INVALID;
    std::unique_lock<std::shared_mutex> g(t->mu);
    // Everything that allocates comes first, so that an allocation failure applies nothing.
    // Entries live after the call: the deletions, then the puts, over the addresses the call names.
    std::map<TxKey, TxTouch> now;
    int64_t live = (int64_t)t->hosts.size();
    auto touch = [&](const neb_tx_addr& a, bool to) {
        const TxKey k = tx_key(a);
        auto it = now.find(k);
        if (it == now.end()) it = now.emplace(k, TxTouch{t->hosts.count(k) != 0, -1}).first;
        live += (int)to - (int)it->second.live;
        it->second.live = to;
    };
    for (uint32_t i = 0; i < ndel; i++) touch(del[i], false);
    for (uint32_t i = 0; i < nput; i++) touch(put[i].addr, true);
    if (live > (int64_t)t->host_cap) return NEB_ERR_NO_KEY_SLOT;
    std::map<TxKey, uint32_t> add;  // the puts' last word per address, as nodes ready to move into hosts
    for (uint32_t i = 0; i < nput; i++) add[tx_key(put[i].addr)] = put[i].tunnel;
    // every put takes a slot; past 3/4 of the slots in use the table is rebuilt without its tombstones
    const bool rebuild = (uint64_t)t->used + nput > (uint64_t)(t->mask + 1u) / 4u * 3u;
    std::vector<std::pair<uint32_t, bool>> fresh;
    std::vector<uint32_t> dead;
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
    if (!rebuild) tx_apply(t, del, ndel, put, nput, &now, &fresh, &dead);
    for (uint32_t i = 0; i < ndel; i++) t->hosts.erase(tx_key(del[i]));
    while (!add.empty()) {
        auto node = add.extract(add.begin());
        auto it = t->hosts.find(node.key());
        if (it != t->hosts.end()) it->second = node.mapped();
        else t->hosts.insert(std::move(node));
    }
    if (rebuild) tx_rebuild_slots(t);
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        if (rebuild) return tx_push_rebuild(t, (hipStream_t)stream);
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

extern "C" NEB_API int neb_tx_table_set_routes(neb_tx_table* t, const neb_route* routes, uint32_t nroutes,
                                               void* stream) try {
    if (!t || (nroutes && !routes)) return NEB_ERR_INVALID;
    std::vector<TxRouteRec> recs;
    std::vector<TxGw> gws;
    TxLens lens{};
    std::set<std::tuple<uint32_t, uint32_t, uint64_t, uint64_t>> seen;
    for (uint32_t i = 0; i < nroutes; i++) {
        const neb_route& r = routes[i];
        if (!cidr_ok(r.prefix) || r.ngateways == 0 || r.ngateways > NEB_ROUTE_MAX_GATEWAYS) return NEB_ERR_INVALID;
        uint64_t total = 0, upto = 0;
        for (uint32_t k = 0; k < r.ngateways; k++) {
            if (!tx_family_ok(r.gateways[k].addr.family)) return NEB_ERR_INVALID;
            total += r.gateways[k].weight;
        }
        if (r.ngateways > 1 && total == 0) return NEB_ERR_INVALID;
        const TxAddr a = tx_addr_from_bytes(r.prefix.addr, r.prefix.family), m = tx_prefix_mask(r.prefix.bits);
        const TxRouteRec rec{r.prefix.family, r.prefix.bits, TxAddr{a.hi & m.hi, a.lo & m.lo}, (uint32_t)gws.size(), r.ngateways};
        if (!seen.emplace(rec.family, rec.bits, rec.addr.hi, rec.addr.lo).second) return NEB_ERR_INVALID;
        recs.push_back(rec);
        for (uint32_t k = 0; k < r.ngateways; k++) {
            upto += r.gateways[k].weight;
            gws.push_back(TxGw{tx_addr_from_bytes(r.gateways[k].addr.addr, r.gateways[k].addr.family), r.gateways[k].addr.family,
                               total ? tx_bucket_bound(upto, total) : 0x7FFFFFFFu});
        }
        tx_lens_add(&lens, rec.family, rec.bits);
    }
    if (recs.size() > t->route_cap || gws.size() > t->gw_cap) return NEB_ERR_NO_KEY_SLOT;
    std::unique_lock<std::shared_mutex> g(t->mu);
    t->routes = std::move(recs);
    t->gws = std::move(gws);
    t->lens = lens;
    tx_rebuild_slots(t);
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        return tx_push_rebuild(t, (hipStream_t)stream);
    }
#endif
    (void)stream;
    return NEB_OK;
} catch (const std::bad_alloc&) {  // thrown while the new set was put together: nothing applied
    return NEB_ERR_INVALID;
}

extern "C" NEB_API int neb_tx_table_set_own(neb_tx_table* t, const neb_cidr* nets, uint32_t n, uint32_t flags) {
    if (!t || n > NEB_INDEX_MAX_NETWORKS || (n && !nets) || (flags & ~(NEB_TX_DROP_LOCAL_BROADCAST | NEB_TX_DROP_MULTICAST)))
        return NEB_ERR_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!cidr_ok(nets[k])) return NEB_ERR_INVALID;
    TxOwn v;
    tx_own_set(&v, nets, n, flags);
    std::unique_lock<std::shared_mutex> g(t->mu);
    t->own = v;
#if defined(__HIPCC__)
    std::lock_guard<std::mutex> dg(t->dev.lock());
    t->down = v;
#endif
    return NEB_OK;
}

extern "C" NEB_API int neb_tx_table_count(const neb_tx_table* t, uint32_t* hosts, uint32_t* routes) {
    if (!t || !hosts || !routes) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    *hosts = (uint32_t)t->hosts.size();
    *routes = (uint32_t)t->routes.size();
    return NEB_OK;
}

extern "C" NEB_API int neb_tx_table_probe(const neb_tx_table* t, uint32_t kind, const neb_cidr* key, uint32_t out[3]) {
    if (!t || !key || !out || kind > NEB_TX_KIND_ROUTE || !tx_family_ok(key->family)) return NEB_ERR_INVALID;
    if (kind == NEB_TX_KIND_ROUTE && !cidr_ok(*key)) return NEB_ERR_INVALID;
    const uint32_t bits = kind == NEB_TX_KIND_ROUTE ? key->bits : 0;
    TxAddr a = tx_addr_from_bytes(key->addr, key->family);
    if (kind == NEB_TX_KIND_ROUTE) {
        const TxAddr m = tx_prefix_mask(bits);
        a = TxAddr{a.hi & m.hi, a.lo & m.lo};
    }
    std::shared_lock<std::shared_mutex> g(t->mu);
    out[0] = tx_find_host(t, kind, key->family, bits, a, &out[1], &out[2]);
    return NEB_OK;
}

extern "C" NEB_API int neb_tx_resolve_batch_host(const neb_tx_table* t, neb_tx_packet* pk, uint32_t n, const uint8_t* in,
                                                 size_t in_len, neb_fw_packet* fw, int32_t* status) {
    if (!t || (n && !pk)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if (pk[i].in_off > in_len || pk[i].len > in_len - pk[i].in_off || (pk[i].len && !in)) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* d = in + pk[i].in_off;
        auto byte = [&](uint32_t k) -> uint32_t { return d[k]; };
        auto look = [&](uint32_t kind, uint32_t family, uint32_t bits, const TxAddr& a, uint64_t* v) {
            return tx_lookup(t->slots.data(), t->mask, kind, family, bits, a, HostLoad{}, v);
        };
        auto gw = [&](uint32_t k) { return t->gws[k]; };
        TxResult r;
        tx_resolve_one(pk[i].len, byte, t->own, t->lens, look, gw, &r);
        pk[i].tunnel = r.tunnel;
        if (status) status[i] = r.status;
        if (fw) std::memcpy(&fw[i], r.fw, sizeof(neb_fw_packet));
    }
    return NEB_OK;
}

extern "C" NEB_API int neb_tx_resolve_batch(neb_engine* e, const neb_tx_table* t, neb_tx_packet* d_pk, uint32_t n,
                                            const uint8_t* d_in, neb_fw_packet* d_fw, int32_t* d_status, void* stream) {
#if defined(__HIPCC__)
    if (!e || !t || t->device < 0 || t->device != neb_engine_device_of(e) || (n && (!d_pk || !d_in)) ||
        (reinterpret_cast<uintptr_t>(d_fw) & 15u))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    // the mirror's lock only: a rebuild or route replacement in progress holds mu and does not stall this call
    DeviceGuard dg(t->device);
    return t->dev.read((hipStream_t)stream, [&](int k, const TxSlot* image) {
        return neb_txt_resolve(image, t->mask, t->dgw[k], &t->dlens[k], &t->down, d_pk, n, d_in, d_fw, d_status, (hipStream_t)stream);
    });
#else
    (void)e, (void)t, (void)d_pk, (void)n, (void)d_in, (void)d_fw, (void)d_status, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}
