// queue.cpp — the C ABI of the submission queue (include/nebula_aead.h): queue_core.hpp's state
// machine over the engine. Staging is pinned, mapped host memory; each batch is one zero-copy
// kernel launch on its own stream (and mixed-key scheduler workspace).
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "engine_internal.hpp"
#include "hip_guard.hpp"
#include "queue_core.hpp"

namespace {

// One stream and mixed-key scheduler workspace per staging batch: consecutive batches run
// concurrently on the device (a small zero-copy batch is PCIe latency, not bandwidth). A batch is
// done when its stream has drained: only that batch is ever on it (a staging batch is relaunched
// only after every submitter has copied its results out), and the stream synchronize makes the
// kernel's stores into the mapped staging visible to the host, as for the zero-copy host batch.
struct HipDev {
    using Token = uint32_t;  // the staging batch's index (its stream)
    neb_engine* e = nullptr;
    int alg = 0, open = 0;
    struct Slot {  // of a staging batch: its stream and workspace, and what its arena, desc and status point at
        neb::Stream stream;
        SchedSpacePtr sched;
        neb::PinnedBuf<> arena;
        neb::PinnedBuf<neb_desc> desc;
        neb::PinnedBuf<int32_t> status;
    };
    std::vector<Slot> slot;
    int launch(uint32_t i, neb_desc* desc, uint32_t n, uint8_t* arena, int32_t* status, uint32_t hint, Token& tok) {
        tok = i;
        DeviceGuard dg(neb_engine_device_of(e));  // (the flusher thread launches)
        return neb_launch(e, {.alg = alg, .open = open, .desc = desc, .n = n, .arena = arena, .status = status,
                              .key_hint = hint, .stream = slot[i].stream, .sched = slot[i].sched.get()});
    }
    int wait(Token& tok) { return hipStreamSynchronize(slot[tok].stream) == hipSuccess ? NEB_OK : NEB_ERR_HIP; }
    bool key_ok(uint32_t key) { return neb_key_alg(e, key) == alg; }
    bool mapped(const uint8_t* arena) { return neb_host_mapped(arena); }
};

}  // namespace

struct neb_queue : neb_q::Queue<HipDev> {};

extern "C" {

NEB_API int neb_queue_create(neb_engine* e, int alg, int open, const neb_queue_config* cfg, neb_queue** out) {
    if (!e || !out || (alg != NEB_ALG_AESGCM && alg != NEB_ALG_CHACHAPOLY) || (open != 0 && open != 1))
        return NEB_ERR_INVALID;
    *out = nullptr;
    neb_queue_config c = cfg ? *cfg : neb_queue_config{};
    if (!neb_q::normalize(c)) return NEB_ERR_INVALID;
    DeviceGuard dg(neb_engine_device_of(e));
    std::unique_ptr<neb_queue> q(new (std::nothrow) neb_queue);  // (a failure below releases it under the guard)
    if (!q) return NEB_ERR_INVALID;
    HipDev& dev = q->dev;
    dev.e = e;
    dev.alg = alg;
    dev.open = open;
    q->open = open;
    q->cfg = c;
    q->b.resize(c.depth);
    dev.slot.resize(c.depth);
    for (uint32_t i = 0; i < c.depth; i++) {
        HipDev::Slot& st = dev.slot[i];
        st.sched.reset(neb_sched_space_new());
        if (st.stream.create(hipStreamNonBlocking) != hipSuccess || !st.sched ||
            st.arena.reserve(c.arena_bytes) != hipSuccess ||
            st.desc.reserve((size_t)c.max_packets * sizeof(neb_desc)) != hipSuccess ||
            st.status.reserve((size_t)c.max_packets * 4) != hipSuccess)
            return NEB_ERR_HIP;
        q->b[i].arena = st.arena;
        q->b[i].desc = st.desc;
        q->b[i].status = st.status;
    }
    q->start();
    *out = q.release();
    return NEB_OK;
}

NEB_API int neb_queue_destroy(neb_queue* q) {
    if (!q) return NEB_ERR_INVALID;
    q->shutdown();
    DeviceGuard dg(neb_engine_device_of(q->dev.e));
    for (const HipDev::Slot& st : q->dev.slot)
        if (st.stream) hipStreamSynchronize(st.stream);
    delete q;  // each slot's staging, workspace and then stream release themselves (hip_owned.hpp)
    return NEB_OK;
}

NEB_API int neb_queue_flush(neb_queue* q) { return q ? q->flush() : NEB_ERR_INVALID; }

NEB_API int neb_queue_stats(neb_queue* q, uint64_t stats[4]) {
    if (!q || !stats) return NEB_ERR_INVALID;
    q->stats(stats);
    return NEB_OK;
}

NEB_API int neb_queue_phases(neb_queue* q, uint64_t ns[6]) {
    if (!q || !ns) return NEB_ERR_INVALID;
    q->phases(ns);
    return NEB_OK;
}

NEB_API int neb_queue_submit(neb_queue* q, const neb_desc* desc, uint32_t n, uint8_t* arena, size_t arena_len,
                             int32_t* status) {
    return q ? q->submit(desc, n, arena, arena_len, status) : NEB_ERR_INVALID;
}

}  // extern "C"
