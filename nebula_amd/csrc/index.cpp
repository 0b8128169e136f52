// index.cpp — neb_index_table_* and neb_rx_resolve_batch[_host]: the table of the hostmap's
// receive-side index lookups (rules: index_core.hpp). The host copy is authoritative: every update
// is applied to it first, under the table's lock, and neb_rx_resolve_batch_host reads it. A table
// made with an engine also keeps two images in device memory: the active one is brought up to date
// by a scatter kernel on the caller's stream (resolve.hip), the spare one takes the next rebuild.
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

#if defined(__HIPCC__)
#include "engine_internal.hpp"
#include "hip_guard.hpp"
#include "resolve.hpp"
#endif

using namespace neb;

namespace {

constexpr uint32_t kIdxMaxCapacity = 1u << 24;
#if defined(__HIPCC__)
constexpr uint32_t kIdxStageOps = 4096;  // ops per scatter launch (two pinned staging buffers)

struct IdxUse {  // the last work a stream has enqueued on an image
    hipStream_t s;
    neb::Event ev;
};
#endif

struct IdxHostLoad {
    uint64_t operator()(const uint64_t* p) const { return *p; }
};

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
    // dmu: which image is active, and the events (taken inside mu by writers, alone by resolves)
    mutable std::mutex dmu;
    DevBuf<IdxSlot> image[2];
    int active = 0;
    mutable std::vector<IdxUse> uses[2];
    PinnedBuf<IdxOp> stage[2];
    Event stage_ev[2];
    bool stage_busy[2] = {false, false};
    int stage_next = 0;
    PinnedBuf<IdxSlot> upload;  // a rebuilt image on its way to the device
    Event update_ev;
    hipStream_t update_stream = nullptr;
    bool update_pending = false;
#endif
};

namespace {

inline bool idx_find_host(const neb_index_table* t, uint32_t space, uint32_t index, uint32_t* slot, uint32_t* probes) {
    return idx_find(t->slots.data(), t->mask, space, index, IdxHostLoad{}, slot, probes);
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

// Entries live after the call: the deletions, then the puts, over the keys the call names.
uint64_t idx_live_after(const neb_index_table* t, const neb_index_key* del, uint32_t ndel, const neb_index_entry* put,
                        uint32_t nput) {
    std::unordered_map<uint64_t, bool> now;
    int64_t delta = 0;
    auto touch = [&](uint32_t space, uint32_t index, bool to) {
        const uint64_t tag = idx_tag(space, index);
        auto it = now.find(tag);
        if (it == now.end()) {
            uint32_t s, p;
            it = now.emplace(tag, idx_find_host(t, space, index, &s, &p)).first;
        }
        delta += (int)to - (int)it->second;
        it->second = to;
    };
    for (uint32_t i = 0; i < ndel; i++) touch(del[i].space, del[i].index, false);
    for (uint32_t i = 0; i < nput; i++) touch(put[i].space, put[i].index, true);
    return (uint64_t)((int64_t)t->live + delta);
}

// The update on the host copy, slot by slot. fresh: the slots it filled, and whether each is still
// live at the end; dead: the slots live before the call that it tombstoned.
void idx_apply(neb_index_table* t, const neb_index_key* del, uint32_t ndel, const neb_index_entry* put, uint32_t nput,
               std::map<uint32_t, bool>* fresh, std::vector<uint32_t>* dead) {
    auto bury = [&](uint32_t s) {
        t->slots[s].tag = kIdxTomb;
        t->live--;
        auto it = fresh->find(s);
        if (it != fresh->end()) it->second = false;
        else dead->push_back(s);
    };
    uint32_t s, p;
    for (uint32_t i = 0; i < ndel; i++)
        if (idx_find_host(t, del[i].space, del[i].index, &s, &p)) bury(s);
    for (uint32_t i = 0; i < nput; i++) {
        const bool had = idx_find_host(t, put[i].space, put[i].index, &s, &p);
        const uint32_t to = idx_free_slot(t, put[i].space, put[i].index);  // behind the old record
        t->slots[to] = IdxSlot{idx_tag(put[i].space, put[i].index), idx_pack_a(put[i]), idx_pack_b(put[i]), 0};
        t->live++;
        t->used++;
        (*fresh)[to] = true;
        if (had) bury(s);
    }
}

// The update through a rebuild of the host copy: the live records re-inserted, no tombstones.
void idx_apply_rebuilt(neb_index_table* t, const neb_index_key* del, uint32_t ndel, const neb_index_entry* put,
                       uint32_t nput) {
    std::map<uint64_t, std::pair<uint64_t, uint64_t>> recs;
    for (const IdxSlot& s : t->slots)
        if (s.tag != kIdxEmpty && s.tag != kIdxTomb) recs[s.tag] = {s.a, s.b};
    for (uint32_t i = 0; i < ndel; i++) recs.erase(idx_tag(del[i].space, del[i].index));
    for (uint32_t i = 0; i < nput; i++) recs[idx_tag(put[i].space, put[i].index)] = {idx_pack_a(put[i]), idx_pack_b(put[i])};
    std::fill(t->slots.begin(), t->slots.end(), IdxSlot{});
    for (const auto& r : recs) {
        const uint32_t space = (uint32_t)(r.first >> 32) & 1u, index = (uint32_t)r.first;
        t->slots[idx_free_slot(t, space, index)] = IdxSlot{r.first, r.second.first, r.second.second, 0};
    }
    t->live = t->used = (uint32_t)recs.size();
}

#if defined(__HIPCC__)
#define IDX_HIP(x)                               \
    do {                                         \
        if ((x) != hipSuccess) return NEB_ERR_HIP; \
    } while (0)

// Record that stream s has work on image k in flight (dmu held).
int idx_note_use(const neb_index_table* t, int k, hipStream_t s) {
    for (IdxUse& u : t->uses[k])
        if (u.s == s) {
            IDX_HIP(hipEventRecord(u.ev, s));
            return NEB_OK;
        }
    Event ev;
    IDX_HIP(ev.create(hipEventDisableTiming));
    t->uses[k].push_back(IdxUse{s, std::move(ev)});
    IDX_HIP(hipEventRecord(t->uses[k].back().ev, s));
    return NEB_OK;
}

// ops to the active image in launches of at most kIdxStageOps, through the two staging buffers.
int idx_scatter_ops(neb_index_table* t, const std::vector<IdxOp>& ops, hipStream_t s) {
    for (size_t at = 0; at < ops.size(); at += kIdxStageOps) {
        const uint32_t cnt = (uint32_t)std::min<size_t>(kIdxStageOps, ops.size() - at);
        const int k = t->stage_next;
        t->stage_next ^= 1;
        if (t->stage_busy[k]) IDX_HIP(hipEventSynchronize(t->stage_ev[k]));  // its last launch has read it
        std::memcpy(t->stage[k], ops.data() + at, (size_t)cnt * sizeof(IdxOp));
        IDX_HIP(neb_idx_scatter(t->image[t->active], t->stage[k], cnt, s));
        IDX_HIP(hipEventRecord(t->stage_ev[k], s));
        t->stage_busy[k] = true;
    }
    return NEB_OK;
}

// The host copy's changes to the active image on s (mu held exclusively).
int idx_push_update(neb_index_table* t, const std::map<uint32_t, bool>& fresh, const std::vector<uint32_t>& dead,
                    hipStream_t s) {
    std::vector<IdxOp> first, second;
    first.reserve(fresh.size());
    for (const auto& f : fresh) {
        const IdxSlot& sl = t->slots[f.first];
        first.push_back(f.second ? IdxOp{f.first, sl.tag, sl.a, sl.b} : IdxOp{f.first, kIdxTomb, 0, 0});
    }
    second.reserve(dead.size());
    for (uint32_t d : dead) second.push_back(IdxOp{d, kIdxTomb, 0, 0});
    if (first.empty() && second.empty()) return NEB_OK;
    std::lock_guard<std::mutex> g(t->dmu);
    // updates take effect in the order of the calls, whatever their streams
    if (t->update_pending && t->update_stream != s) IDX_HIP(hipStreamWaitEvent(s, t->update_ev, 0));
    int rc = idx_scatter_ops(t, first, s);  // new records first: a replaced key is never absent
    if (rc == NEB_OK) rc = idx_scatter_ops(t, second, s);
    if (rc != NEB_OK) return rc;
    IDX_HIP(hipEventRecord(t->update_ev, s));
    t->update_stream = s;
    t->update_pending = true;
    return idx_note_use(t, t->active, s);
}

// The rebuilt host copy into the spare image, then the switch (mu held exclusively). Blocks.
int idx_push_rebuild(neb_index_table* t, hipStream_t s) {
    int spare;
    std::vector<hipEvent_t> waits;
    {
        std::lock_guard<std::mutex> g(t->dmu);
        spare = t->active ^ 1;
        for (const IdxUse& u : t->uses[spare]) waits.push_back(u.ev);  // nothing new can start on the spare image
    }
    for (hipEvent_t ev : waits) IDX_HIP(hipEventSynchronize(ev));
    const size_t bytes = t->slots.size() * sizeof(IdxSlot);
    std::memcpy(t->upload, t->slots.data(), bytes);
    IDX_HIP(hipMemcpyAsync(t->image[spare], t->upload, bytes, hipMemcpyHostToDevice, s));
    IDX_HIP(hipStreamSynchronize(s));  // complete before any stream can be pointed at it
    std::lock_guard<std::mutex> g(t->dmu);
    t->active = spare;
    t->update_pending = false;  // later updates go to this image, which nothing else writes
    return NEB_OK;
}

// Waits for the device work on the table, then deletes it: its members release themselves
// (hip_owned.hpp), with the table's device current.
void idx_delete_device(neb_index_table* t) {
    DeviceGuard dg(t->device);
    for (int k = 0; k < 2; k++) {
        for (IdxUse& u : t->uses[k]) (void)hipEventSynchronize(u.ev);
        if (t->stage_ev[k]) (void)hipEventSynchronize(t->stage_ev[k]);
    }
    if (t->update_ev) (void)hipEventSynchronize(t->update_ev);
    delete t;
}

int idx_init_device(neb_index_table* t) {
    const size_t bytes = t->slots.size() * sizeof(IdxSlot);
    for (int k = 0; k < 2; k++) {
        IDX_HIP(t->image[k].reserve(bytes));
        IDX_HIP(hipMemset(t->image[k], 0, bytes));
        IDX_HIP(t->stage[k].reserve(kIdxStageOps * sizeof(IdxOp)));
        IDX_HIP(t->stage_ev[k].create(hipEventDisableTiming));
    }
    IDX_HIP(t->upload.reserve(bytes));
    IDX_HIP(t->update_ev.create(hipEventDisableTiming));
    IDX_HIP(hipDeviceSynchronize());  // the images are zero before any stream reads them
    return NEB_OK;
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
        const int rc = idx_init_device(t);
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
                                              const neb_index_entry* put, uint32_t nput, void* stream) {
    if (!t) return NEB_ERR_INVALID;
    const int rc = idx_validate(del, ndel, put, nput);
    if (rc != NEB_OK) return rc;
    std::unique_lock<std::shared_mutex> g(t->mu);
    if (idx_live_after(t, del, ndel, put, nput) > t->capacity) return NEB_ERR_NO_KEY_SLOT;
    // every put takes a slot; past 3/4 of the slots in use the table is rebuilt without its tombstones
    const bool rebuild = (uint64_t)t->used + nput > (uint64_t)(t->mask + 1u) / 4u * 3u;
    std::map<uint32_t, bool> fresh;
    std::vector<uint32_t> dead;
    if (rebuild) idx_apply_rebuilt(t, del, ndel, put, nput);
    else idx_apply(t, del, ndel, put, nput, &fresh, &dead);
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        return rebuild ? idx_push_rebuild(t, (hipStream_t)stream) : idx_push_update(t, fresh, dead, (hipStream_t)stream);
    }
#endif
    (void)stream;
    return NEB_OK;
}

extern "C" NEB_API int neb_index_table_set_own_networks(neb_index_table* t, const neb_cidr* nets, uint32_t n,
                                                        void* stream) {
    (void)stream;
    if (!t || n > NEB_INDEX_MAX_NETWORKS || (n && !nets)) return NEB_ERR_INVALID;
    for (uint32_t k = 0; k < n; k++)
        if (!idx_cidr_ok(nets[k])) return NEB_ERR_INVALID;
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
            return idx_lookup(t->slots.data(), t->mask, space, index, IdxHostLoad{}, want_route, r);
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
    std::lock_guard<std::mutex> g(t->dmu);
    const int k = t->active;
    IDX_HIP(neb_idx_resolve(t->image[k], t->mask, &nets, d_pk, d_src, n, d_arena, d_route, d_via, (hipStream_t)stream));
    return idx_note_use(t, k, (hipStream_t)stream);  // a rebuild into this image waits for it
#else
    (void)e, (void)t, (void)d_pk, (void)d_src, (void)n, (void)d_arena, (void)d_route, (void)d_via, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}
