// conntrack.cpp — neb_conntrack_*: the connection table (rules: conntrack_core.hpp). A table made with
// an engine keeps its image in device memory only: the device changes it with every batch, so there
// is no host copy to keep or to upload (no table_mirror.hpp), and the calls here check their
// arguments, order the table's work and enqueue conntrack.hip's launches. A host-only table keeps the
// same image in host memory and the _host calls run the same rules over it, one element after the
// other. Compiled without HIP (g++: tests/sanitize_conntrack) only the host-only table exists.
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "conntrack_core.hpp"

#if defined(__HIPCC__)
#include "conntrack.hpp"
#include "engine_internal.hpp"
#include "hip_guard.hpp"
#include "hip_owned.hpp"
#include "workspace.hpp"
#endif

using namespace neb;

struct neb_conntrack {
    CtParams p{};
    uint32_t max_batch = 0;
    std::atomic<uint32_t> version{0};
    // host-only table
    std::vector<CtSlot> slots;
    uint64_t counters[2] = {0, 0};  // live, tombstones
#if defined(__HIPCC__)
    int device = -1;  // -1: host-only
    // mu: the launch order of the table's calls and the fields below
    std::mutex mu;
    DevBuf<CtSlot> image[2];  // the live one is image[cur]; the other exists during a compaction only
    int cur = 0;
    DevBuf<uint64_t> dcounters;
    CtWs ws{};
    HipWorkspace<> look;  // the lookups' workspace: one lookup at a time
    HipWorkspace<> mut;   // no memory: the event behind the last add, evict or compaction
#endif
};

namespace {

inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) & (a - 1u); }

#if defined(__HIPCC__)
#define CT_TRY(x)                                  \
    do {                                           \
        if ((x) != hipSuccess) return NEB_ERR_HIP; \
    } while (0)

void ct_delete_device(neb_conntrack* t) {
    DeviceGuard dg(t->device);
    t->look.destroy();  // each waits for its last batch
    t->mut.destroy();
    delete t;
}

int ct_init_device(neb_conntrack* t) {
    const size_t bytes = ((size_t)t->p.mask + 1u) * sizeof(CtSlot);
    CT_TRY(t->image[0].reserve(bytes));
    CT_TRY(hipMemset(t->image[0], 0, bytes));
    CT_TRY(t->dcounters.reserve(64));
    CT_TRY(hipMemset(t->dcounters, 0, 64));
    size_t cub = 0;
    const size_t ws_bytes = neb_ct_ws_bytes(t->max_batch, &cub);
    CT_TRY(t->look.reserve(ws_bytes));
    CT_TRY(hipMemset(t->look.mem(), 0, ws_bytes));
    ct_ws_layout(t->max_batch, cub, t->look.mem(), &t->ws);
    return NEB_OK;
}

// A device call's table: made with this engine.
inline bool ct_device_ok(const neb_engine* e, const neb_conntrack* t) {
    return e && t && t->device >= 0 && t->device == neb_engine_device_of(e);
}
#endif

}  // namespace

extern "C" NEB_API int neb_conntrack_create(neb_engine* e, uint32_t capacity, uint64_t seed, uint64_t tcp_ns, uint64_t udp_ns,
                                            uint64_t default_ns, uint32_t max_batch, neb_conntrack** out) {
    if (!out || capacity == 0 || capacity > kCtMaxCapacity || max_batch == 0 || max_batch > 0x3FFFFFFFu) return NEB_ERR_INVALID;
    *out = nullptr;
#if !defined(__HIPCC__)
    if (e) return NEB_ERR_NO_DEVICE;
#endif
    neb_conntrack* t = new (std::nothrow) neb_conntrack;
    if (!t) return NEB_ERR_INVALID;
    t->p = CtParams{seed, tcp_ns, udp_ns, default_ns, ct_slots_for(capacity) - 1u, capacity};
    t->max_batch = max_batch;
#if defined(__HIPCC__)
    if (e) {
        t->device = neb_engine_device_of(e);
        DeviceGuard dg(t->device);
        const int rc = ct_init_device(t);
        if (rc != NEB_OK) {
            ct_delete_device(t);
            return rc;
        }
        *out = t;
        return NEB_OK;
    }
#endif
    try {
        t->slots.assign((size_t)t->p.mask + 1u, CtSlot{});
    } catch (const std::bad_alloc&) {
        delete t;
        return NEB_ERR_INVALID;
    }
    *out = t;
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_destroy(neb_conntrack* t) {
    if (!t) return NEB_ERR_INVALID;
#if defined(__HIPCC__)
    if (t->device >= 0) {
        ct_delete_device(t);
        return NEB_OK;
    }
#endif
    delete t;
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_set_rules_version(neb_conntrack* t, uint16_t v) {
    if (!t) return NEB_ERR_INVALID;
    t->version.store(v, std::memory_order_release);
    return NEB_OK;
}

// ---- the host forms ------------------------------------------------------------------------------

extern "C" NEB_API int neb_conntrack_lookup_batch_host(neb_conntrack* t, const neb_fw_packet* fw, int32_t* status, uint32_t n,
                                                       uint64_t now_ns, uint8_t* verdict, neb_plain_packet* plain,
                                                       neb_tx_packet* tx, neb_ct_work* work, uint32_t work_cap, uint32_t* counts) {
    if (!t || t->slots.empty() || n > t->max_batch || !counts || (n && (!fw || !status || !verdict)) || (work_cap && !work))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    const uint32_t version = t->version.load(std::memory_order_acquire);
    uint32_t c[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < n; i++) {
        uint32_t v = NEB_CT_NONE;
        if (status[i] == NEB_STATUS_OK) {
            v = ct_lookup_one(t->slots.data(), t->p, version, now_ns, ct_key_of(&fw[i]), CtHostMem{});
            c[(v & 0x7Fu) - 1u]++;
            if (v != NEB_CT_HIT) {
                if (plain || tx) status[i] = NEB_STATUS_FW_HELD;
                if (plain) {  // the ABI aligns the records of the host forms to nothing
                    uint8_t* flags = reinterpret_cast<uint8_t*>(&plain[i]) + offsetof(neb_plain_packet, flags);
                    *flags |= NEB_PLAIN_SKIP;
                }
                if (tx) {
                    const uint32_t none = NEB_TX_NO_TUNNEL;
                    std::memcpy(reinterpret_cast<uint8_t*>(&tx[i]) + offsetof(neb_tx_packet, tunnel), &none, 4);
                }
                if (c[3] < work_cap) {
                    neb_ct_work w{};
                    w.packet = i;
                    w.verdict = v;
                    std::memcpy(&w.fw, &fw[i], sizeof w.fw);
                    std::memcpy(&work[c[3]], &w, sizeof w);
                }
                c[3]++;
            }
        }
        verdict[i] = (uint8_t)v;
    }
    std::memcpy(counts, c, sizeof c);
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_add_batch_host(neb_conntrack* t, const neb_fw_packet* keys, const uint8_t* incoming,
                                                    uint32_t n, uint64_t now_ns, neb_ct_result* result) {
    if (!t || t->slots.empty() || n > t->max_batch || (n && (!keys || !incoming || !result))) return NEB_ERR_INVALID;
    const uint32_t version = t->version.load(std::memory_order_acquire);
    auto key_of = [&](uint32_t j) { return ct_key_of(&keys[j < n ? j : 0]); };
    // the device's two launches, one element after the other
    for (uint32_t i = 0; i < n; i++) {
        const CtAdd r = ct_add_claim(t->slots.data(), &t->counters[0], t->p, version, now_ns, i, key_of(i), incoming[i], key_of,
                                     CtHostMem{});
        std::memcpy(&result[i], &r, sizeof r);
    }
    auto code_of = [&](uint32_t j) {
        CtAdd o;
        std::memcpy(&o, &result[j < n ? j : 0], sizeof o);
        return o.code;
    };
    for (uint32_t i = 0; i < n; i++) {
        CtAdd r;
        std::memcpy(&r, &result[i], sizeof r);
        const CtAdd f = ct_add_settle(t->slots.data(), t->counters, r, code_of, CtHostMem{});
        std::memcpy(&result[i], &f, sizeof f);
    }
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_evict_batch_host(neb_conntrack* t, const neb_fw_packet* keys, uint32_t n, uint64_t now_ns,
                                                      int force, int64_t* remaining) {
    if (!t || t->slots.empty() || n > t->max_batch || (n && (!keys || !remaining))) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const int64_t r = ct_evict_one(t->slots.data(), t->counters, t->p, now_ns, force != 0, ct_key_of(&keys[i]), CtHostMem{});
        std::memcpy(&remaining[i], &r, sizeof r);
    }
    return NEB_OK;
}

// ---- the device forms ----------------------------------------------------------------------------

extern "C" NEB_API int neb_conntrack_lookup_batch(neb_engine* e, neb_conntrack* t, const neb_fw_packet* d_fw, int32_t* d_status,
                                                  uint32_t n, uint64_t now_ns, uint8_t* d_verdict, neb_plain_packet* d_plain,
                                                  neb_tx_packet* d_tx, neb_ct_work* d_work, uint32_t work_cap, uint32_t* d_counts,
                                                  void* stream) {
#if defined(__HIPCC__)
    if (!ct_device_ok(e, t) || n > t->max_batch || !d_counts || (n && (!d_fw || !d_status || !d_verdict)) ||
        (work_cap && !d_work) || misaligned(d_fw, 16) || misaligned(d_work, 16) || misaligned(d_plain, 16) ||
        misaligned(d_tx, 8) || misaligned(d_status, 4) || misaligned(d_counts, 4))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    DeviceGuard dg(t->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(t->mu);
    CT_TRY(t->look.begin(s));
    const CtLookupArgs a{t->image[t->cur], d_fw, d_status, d_verdict, d_plain, d_tx, d_work, d_counts, now_ns, t->p, n,
                         t->version.load(std::memory_order_acquire), work_cap, t->ws};
    CT_TRY(neb_ct_lookup(&a, s));
    CT_TRY(t->look.end(s));
    return NEB_OK;
#else
    (void)e, (void)t, (void)d_fw, (void)d_status, (void)n, (void)now_ns, (void)d_verdict, (void)d_plain, (void)d_tx, (void)d_work,
        (void)work_cap, (void)d_counts, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}

extern "C" NEB_API int neb_conntrack_add_batch(neb_engine* e, neb_conntrack* t, const neb_fw_packet* d_keys,
                                               const uint8_t* d_incoming, uint32_t n, uint64_t now_ns, neb_ct_result* d_result,
                                               void* stream) {
#if defined(__HIPCC__)
    if (!ct_device_ok(e, t) || n > t->max_batch || (n && (!d_keys || !d_incoming || !d_result)) || misaligned(d_keys, 16) ||
        misaligned(d_result, 4))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    DeviceGuard dg(t->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(t->mu);
    CT_TRY(t->mut.begin(s));
    const CtAddArgs a{t->image[t->cur], t->dcounters, d_keys, d_incoming, d_result, now_ns, t->p, n,
                      t->version.load(std::memory_order_acquire)};
    CT_TRY(neb_ct_add(&a, s));
    CT_TRY(t->mut.end(s));
    return NEB_OK;
#else
    (void)e, (void)t, (void)d_keys, (void)d_incoming, (void)n, (void)now_ns, (void)d_result, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}

extern "C" NEB_API int neb_conntrack_evict_batch(neb_engine* e, neb_conntrack* t, const neb_fw_packet* d_keys, uint32_t n,
                                                 uint64_t now_ns, int force, int64_t* d_remaining, void* stream) {
#if defined(__HIPCC__)
    if (!ct_device_ok(e, t) || n > t->max_batch || (n && (!d_keys || !d_remaining)) || misaligned(d_keys, 16) ||
        misaligned(d_remaining, 8))
        return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    DeviceGuard dg(t->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(t->mu);
    CT_TRY(t->mut.begin(s));
    const CtEvictArgs a{t->image[t->cur], t->dcounters, d_keys, d_remaining, now_ns, t->p, n, force ? 1u : 0u};
    CT_TRY(neb_ct_evict(&a, s));
    CT_TRY(t->mut.end(s));
    return NEB_OK;
#else
    (void)e, (void)t, (void)d_keys, (void)n, (void)now_ns, (void)force, (void)d_remaining, (void)stream;
    return NEB_ERR_NO_DEVICE;
#endif
}

// ---- compaction, count and the tests' views ------------------------------------------------------

extern "C" NEB_API int neb_conntrack_compact(neb_conntrack* t, void* stream) {
    if (!t) return NEB_ERR_INVALID;
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        hipStream_t s = (hipStream_t)stream;
        std::lock_guard<std::mutex> g(t->mu);
        CT_TRY(t->look.sync());  // whatever still reads or writes the live image
        CT_TRY(t->mut.sync());
        const size_t bytes = ((size_t)t->p.mask + 1u) * sizeof(CtSlot);
        const int spare = 1 - t->cur;
        CT_TRY(t->image[spare].reserve(bytes));
        CT_TRY(hipMemsetAsync(t->image[spare], 0, bytes, s));
        CT_TRY(neb_ct_rehash(t->image[t->cur], t->image[spare], t->dcounters, &t->p, s));
        CT_TRY(hipStreamSynchronize(s));
        t->image[t->cur].reset();
        t->cur = spare;
        return NEB_OK;
    }
#endif
    (void)stream;
    try {
        std::vector<CtSlot> fresh((size_t)t->p.mask + 1u, CtSlot{});
        for (const CtSlot& old : t->slots) ct_rehash_one(&old, fresh.data(), t->p, CtHostMem{});
        t->slots.swap(fresh);
        t->counters[1] = 0;
    } catch (const std::bad_alloc&) {
        return NEB_ERR_INVALID;
    }
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_count(neb_conntrack* t, uint64_t out[3]) {
    if (!t || !out) return NEB_ERR_INVALID;
    out[2] = (uint64_t)t->p.mask + 1u;
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        std::lock_guard<std::mutex> g(t->mu);
        CT_TRY(t->look.sync());
        CT_TRY(t->mut.sync());
        CT_TRY(hipMemcpy(out, t->dcounters, 16, hipMemcpyDeviceToHost));
        return NEB_OK;
    }
#endif
    out[0] = CtHostMem{}.load(&t->counters[0]);
    out[1] = CtHostMem{}.load(&t->counters[1]);
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_home(const neb_conntrack* t, const neb_fw_packet* key, uint32_t* slot) {
    if (!t || !key || !slot) return NEB_ERR_INVALID;
    *slot = ct_home(ct_hash(t->p.seed, ct_key_of(key)), t->p.mask);
    return NEB_OK;
}

extern "C" NEB_API int neb_conntrack_dump(neb_conntrack* t, void* slots_out, uint32_t nslots) {
    if (!t || !slots_out || nslots != t->p.mask + 1u) return NEB_ERR_INVALID;
    const size_t bytes = (size_t)nslots * sizeof(CtSlot);
#if defined(__HIPCC__)
    if (t->device >= 0) {
        DeviceGuard dg(t->device);
        std::lock_guard<std::mutex> g(t->mu);
        CT_TRY(t->look.sync());
        CT_TRY(t->mut.sync());
        CT_TRY(hipMemcpy(slots_out, t->image[t->cur], bytes, hipMemcpyDeviceToHost));
        return NEB_OK;
    }
#endif
    std::memcpy(slots_out, t->slots.data(), bytes);
    return NEB_OK;
}
