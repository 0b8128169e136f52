// index.cpp — neb_index_table_* and neb_rx_resolve_batch[_host]: the table of the hostmap's
// receive-side index lookups (rules: index_core.hpp). The host copy is authoritative: every update
// is applied to it first, under the table's lock, and neb_rx_resolve_batch_host reads it. A table
// made with an engine also keeps a device copy (table_mirror.hpp), written by resolve.hip's scatter.
// Compiled without HIP (g++: tests/sanitize_index) only the host-only table exists.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "index_core.hpp"
#include "table_mirror.hpp"

#if defined(__HIPCC__)
#include "engine_internal.hpp"
#include "hip_guard.hpp"
#include "resolve.hpp"
#endif

using namespace neb;

namespace {

constexpr uint32_t kIdxMaxCapacity = 1u << 24;

struct IdxTouch {  // one key an update names
    bool live;      // is it live now
    int32_t fresh;  // the slot this call filled for it, as an index into `fresh`, or -1
};
using IdxRecs = std::map<uint64_t, std::pair<uint64_t, uint64_t>>;  // tag -> a, b

}  // namespace

struct neb_index_table {
    uint32_t capacity = 0, mask = 0;
    // mu: the host copy, the networks and, for writers, the order of the updates' device work
    mutable std::shared_mutex mu;
    std::vector<IdxSlot> slots;
    uint32_t live = 0, used = 0;  // used: live + tombstones
    IdxNets nets{};
#if defined(__HIPCC__)
    int device = -1;  // -1: host-only
    // the device copy; its lock is taken inside mu by writers, alone by the resolve's launch
    TableMirror<HipWsApi, IdxSlot, IdxOp> dev;
#endif
};

namespace {

inline bool idx_find_host(const neb_index_table* t, uint32_t space, uint32_t index, uint32_t* slot, uint32_t* probes) {
    return idx_find(t->slots.data(), t->mask, space, index, HostLoad{}, slot, probes);
}

// The first EMPTY slot of a key's chain (the table always has one).
inline uint32_t idx_free_slot(const neb_index_table* t, uint32_t space, uint32_t index) {
    uint32_t s = idx_hash(space, index) & t->mask;
    while (t->slots[s].tag != kIdxEmpty) s = (s + 1u) & t->mask;
    return s;
}

int idx_validate(const neb_index_key* del, uint32_t ndel, const neb_index_entry* put, uint32_t nput) {
    if ((ndel && !del) || (nput && !put)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < ndel; i++)
        if (del[i].space > NEB_INDEX_RELAY) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < nput; i++) {
        if (put[i].space > NEB_INDEX_RELAY) return NEB_ERR_INVALID;
        if (put[i].space == NEB_INDEX_TUNNEL && (put[i].flags != 0 || put[i].route.tunnel != NEB_RELAY_NONE))
            return NEB_ERR_INVALID;
    }
    return NEB_OK;
}

// The update on the host copy, slot by slot. fresh: the slots it filled, and whether each is still
// live at the end; dead: the slots live before the call that it tombstoned. Allocates nothing: the
// caller has reserved fresh and dead, and `now` holds every key the call names.
void idx_apply(neb_index_table* t, const neb_index_key* del, uint32_t ndel, const neb_index_entry* put, uint32_t nput,
               std::unordered_map<uint64_t, IdxTouch>* now, std::vector<std::pair<uint32_t, bool>>* fresh,
               std::vector<uint32_t>* dead) {
    auto bury = [&](uint32_t s, IdxTouch* tc) {
        t->slots[s].tag = kIdxTomb;
        t->live--;
        if (tc->fresh >= 0) (*fresh)[(size_t)tc->fresh].second = false;
        else dead->push_back(s);
        tc->fresh = -1;
    };
    uint32_t s, p;
    for (uint32_t i = 0; i < ndel; i++)
        if (idx_find_host(t, del[i].space, del[i].index, &s, &p)) bury(s, &now->find(idx_tag(del[i].space, del[i].index))->second);
    for (uint32_t i = 0; i < nput; i++) {
        IdxTouch* tc = &now->find(idx_tag(put[i].space, put[i].index))->second;
        const bool had = idx_find_host(t, put[i].space, put[i].index, &s, &p);
        const uint32_t to = idx_free_slot(t, put[i].space, put[i].index);  // behind the old record
        t->slots[to] = IdxSlot{idx_tag(put[i].space, put[i].index), idx_pack_a(put[i]), idx_pack_b(put[i]), 0};
        t->live++;
        t->used++;
        fresh->emplace_back(to, true);
        if (had) bury(s, tc);
        tc->fresh = (int32_t)fresh->size() - 1;
    }
    std::sort(fresh->begin(), fresh->end());  // the device ops go out in slot order
}

// The live records after the update, in tag order: what a rebuild re-inserts.
IdxRecs idx_records_after(const neb_index_table* t, const neb_index_key* del, uint32_t ndel, const neb_index_entry* put,
                          uint32_t nput) {
    IdxRecs recs;
    for (const IdxSlot& s : t->slots)
        if (s.tag != kIdxEmpty && s.tag != kIdxTomb) recs[s.tag] = {s.a, s.b};
    for (uint32_t i = 0; i < ndel; i++) recs.erase(idx_tag(del[i].space, del[i].index));
    for (uint32_t i = 0; i < nput; i++) recs[idx_tag(put[i].space, put[i].index)] = {idx_pack_a(put[i]), idx_pack_b(put[i])};
    return recs;
}

// The update through a rebuild of the host copy: recs re-inserted, no tombstones. Allocates nothing.
void idx_apply_rebuilt(neb_index_table* t, const IdxRecs& recs) {
    std::fill(t->slots.begin(), t->slots.end(), IdxSlot{});
    for (const auto& r : recs) {
        const uint32_t space = (uint32_t)(r.first >> 32) & 1u, index = (uint32_t)r.first;
        t->slots[idx_free_slot(t, space, index)] = IdxSlot{r.first, r.second.first, r.second.second, 0};
    }
    t->live = t->used = (uint32_t)recs.size();
}

#if defined(__HIPCC__)
// Waits for the device work on the table, then deletes it: its members release themselves, with
// the table's device current.
void idx_delete_device(neb_index_table* t) {
    DeviceGuard dg(t->device);
    t->dev.drain();
    delete t;
}
#endif

}  // namespace

extern "C" NEB_API int neb_index_table_create(neb_engine* e, uint32_t capacity, neb_index_table** out) {
    if (!out || capacity == 0 || capacity > kIdxMaxCapacity) return NEB_ERR_INVALID;
    *out = nullptr;
#if !defined(__HIPCC__)
    if (e) return NEB_ERR_NO_DEVICE;
#endif
    neb_index_table* t = new (std::nothrow) neb_index_table;
    if (!t) return NEB_ERR_INVALID;
    t->capacity = capacity;
    t->slots.assign(idx_slots_for(capacity), IdxSlot{});
    t->mask = (uint32_t)t->slots.size() - 1u;
#if defined(__HIPCC__)
    if (e) {
        t->device = neb_engine_device_of(e);
        DeviceGuard dg(t->device);
        const int rc = t->dev.init(t->slots.size());
        if (rc != NEB_OK) {
            idx_delete_device(t);
            return rc;
        }
    }
#endif
    *out = t;
    return NEB_OK;
}

extern "C" NEB_API int neb_index_table_destroy(neb_index_table* t) {
    if (!t) return NEB_ERR_INVALID;
#if defined(__HIPCC__)
    if (t->device >= 0) {
        idx_delete_device(t);
        return NEB_OK;
    }
#endif
    delete t;
    return NEB_OK;
}

extern "C" NEB_API int neb_index_table_update(neb_index_table* t, const neb_index_key* del, uint32_t ndel,
                                              const neb_index_entry* put, uint32_t nput, void* stream) try {
    if (!t) return NEB_ERR_INVALID;
    const int rc = idx_validate(del, ndel, put, nput);
    if (rc != NEB_OK) return rc;
    std::unique_lock<std::shared_mutex> g(t->mu);
    // Everything that allocates comes first, so that an allocation failure applies nothing.
    // Entries live after the call: the deletions, then the puts, over the keys the call names.
    std::unordered_map<uint64_t, IdxTouch> now;
    int64_t live = (int64_t)t->live;
    auto touch = [&](uint32_t space, uint32_t index, bool to) {
        const uint64_t tag = idx_tag(space, index);
        auto it = now.find(tag);
        if (it == now.end()) {
            uint32_t s, p;
            it = now.emplace(tag, IdxTouch{idx_find_host(t, space, index, &s, &p), -1}).first;
        }
        live += (int)to - (int)it->second.live;
        it->second.live = to;
    };
    for (uint32_t i = 0; i < ndel; i++) touch(del[i].space, del[i].index, false);
    for (uint32_t i = 0; i < nput; i++) touch(put[i].space, put[i].index, true);
    if (live > (int64_t)t->capacity) return NEB_ERR_NO_KEY_SLOT;
    // every put takes a slot; past 3/4 of the slots in use the table is rebuilt without its tombstones
    const bool rebuild = (uint64_t)t->used + nput > (uint64_t)(t->mask + 1u) / 4u * 3u;
    IdxRecs recs;
    std::vector<std::pair<uint32_t, bool>> fresh;
    std::vector<uint32_t> dead;
    if (rebuild) {
        recs = idx_records_after(t, del, ndel, put, nput);
    } else {
        fresh.reserve(nput);
        dead.reserve((size_t)ndel + nput);
    }
#if defined(__HIPCC__)
    std::vector<IdxOp> first, second;
    if (!rebuild && t->device >= 0) {
        first.reserve(nput);
        second.reserve((size_t)ndel + nput);
    }
#endif
    // From here on nothing allocates on the host.
    if (rebuild) idx_apply_rebuilt(t, recs);
    else idx_apply(t, del, ndel, put, nput, &now, &fresh, &dead);
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        if (rebuild) return t->dev.rebuild(t->slots.data(), (hipStream_t)stream);
        for (const auto& f : fresh) {
            const IdxSlot& sl = t->slots[f.first];
            first.push_back(f.second ? IdxOp{f.first, sl.tag, sl.a, sl.b} : IdxOp{f.first, kIdxTomb, 0, 0});
        }
        for (uint32_t d : dead) second.push_back(IdxOp{d, kIdxTomb, 0, 0});
        return t->dev.update(first, second, (hipStream_t)stream, neb_idx_scatter);
    }
#endif
    (void)stream;
    return NEB_OK;
} catch (const std::bad_alloc&) {
    return NEB_ERR_INVALID;
}

extern "C" NEB_API int neb_index_table_set_own_networks(neb_index_table* t, const neb_cidr* nets, uint32_t n,
                                                        void* stream) {
    (void)stream;
    if (!t || n > NEB_INDEX_MAX_NETWORKS || (n && !nets)) return NEB_ERR_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!cidr_ok(nets[k])) return NEB_ERR_INVALID;
    IdxNets v;
    idx_nets_set(&v, nets, n);
    std::unique_lock<std::shared_mutex> g(t->mu);
    t->nets = v;
    return NEB_OK;
}

extern "C" NEB_API int neb_index_table_count(const neb_index_table* t, uint32_t* live) {
    if (!t || !live) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    *live = t->live;
    return NEB_OK;
}

extern "C" NEB_API int neb_index_table_probe(const neb_index_table* t, uint32_t space, uint32_t index,
                                             uint32_t out[3]) {
    if (!t || !out || space > NEB_INDEX_RELAY) return NEB_ERR_INVALID;
    std::shared_lock<std::shared_mutex> g(t->mu);
    out[0] = idx_find_host(t, space, index, &out[1], &out[2]);
    return NEB_OK;
}

extern "C" NEB_API int neb_rx_resolve_batch_host(const neb_index_table* t, neb_rx_packet* pk, const neb_rx_source* src,
                                                 uint32_t n, const uint8_t* arena, size_t arena_len,
                                                 neb_relay_route* route, neb_rx_via* via) {
    if (!t || (n && !pk)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = idx_rx_len(pk[i]);
        if (pk[i].off > arena_len || len > arena_len - pk[i].off || (len && !arena)) return NEB_ERR_INVALID;
    }
    std::shared_lock<std::shared_mutex> g(t->mu);
    for (uint32_t i = 0; i < n; i++) {
        bool own = false;
        if (src && src[i].family != 0) {
            uint32_t w[4];
            std::memcpy(w, src[i].addr, 16);  // the bytes as little-endian dwords
            own = idx_own_source(t->nets, src[i].family, w);
        }
        auto hdr = [&](uint32_t at, uint32_t* w0, uint32_t* w1) {
            const uint8_t* h = arena + pk[i].off + at;
            std::memcpy(w0, h, 4);
            std::memcpy(w1, h + 4, 4);
        };
        auto look = [&](uint32_t space, uint32_t index, bool want_route, IdxRec* r) {
            return idx_lookup(t->slots.data(), t->mask, space, index, HostLoad{}, want_route, r);
        };
        uint32_t key;
        neb_relay_route r;
        neb_rx_via v;
        idx_resolve_one(idx_rx_len(pk[i]), hdr, look, &key, &r, &v);
        pk[i].key_id = key;
        if (own) pk[i].len |= NEB_RX_OWN_SOURCE;
        if (route) route[i] = r;
        if (via) via[i] = v;
    }
    return NEB_OK;
}

extern "C" NEB_API int neb_rx_resolve_batch(neb_engine* e, const neb_index_table* t, neb_rx_packet* d_pk,
                                            const neb_rx_source* d_src, uint32_t n, const uint8_t* d_arena,
                                            neb_relay_route* d_route, neb_rx_via* d_via, void* stream) {
#if defined(__HIPCC__)
    if (!e || !t || t->device < 0 || t->device != neb_engine_device_of(e) || (n && (!d_pk || !d_arena)))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    IdxNets nets;
    {
        std::shared_lock<std::shared_mutex> g(t->mu);
        nets = t->nets;
    }
    DeviceGuard dg(t->device);
    return t->dev.read((hipStream_t)stream, [&](int, const IdxSlot* image) {
        return neb_idx_resolve(image, t->mask, &nets, d_pk, d_src, n, d_arena, d_route, d_via, (hipStream_t)stream);
    });
#else
    (void)e, (void)t, (void)d_pk, (void)d_src, (void)n, (void)d_arena, (void)d_route, (void)d_via, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}
