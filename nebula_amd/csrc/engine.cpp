// engine.cpp — host side of the C ABI in include/nebula_aead.h.
//
// Owns one HIP device per engine: its stream, the device key table, pinned staging for the
// per-packet CipherState calls, the staged host-resident batch pipeline (Pipe) and the host
// receive's staging (neb::RxStaging). Every seal or open of a batch, whatever path asks for it, is
// one launch_batch over a neb::BatchLaunch (engine_internal.hpp), which window.cpp and queue.cpp
// reach through neb_launch. All packet arithmetic runs in the gfx950 kernels (aes_gcm.hip,
// chacha_poly.hip); there is no CPU path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <cstring>
#include <cxxabi.h>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <unistd.h>
#include <vector>

#include "../../include/nebula_aead.h"
#include "hip_guard.hpp"
#include "knobs.hpp"
#include "host_common.hpp"
#include "layout.hpp"
#include "pipe_core.hpp"
#include "rxwin.hpp"
#include "sched.hpp"
#include "timing.hpp"
#include "tx.hpp"
#include "coalesce.hpp"
#include "recv.hpp"
#include "report.hpp"
#include "send.hpp"
#include "cipher.hpp"
#include "comb_core.hpp"
#include "engine_internal.hpp"

// Device workspace of the mixed-key scheduler (sched.hpp). One per engine (and per queue batch,
// receive slot and window set); batches on different streams never overlap in it (workspace.hpp).
struct SchedSpace {
    neb::HipWorkspace<> dev;
    uint32_t n_cap = 0;
    neb::SchedWs ws{};
    bool dirty = true;  // the bin counts need a clear (new buffer, or a batch that failed to launch)
    std::mutex mu;
};

namespace {

constexpr size_t kStageMin = 1 << 16;
using neb::BatchLaunch;
using neb::DevBuf;
using neb::PinnedBuf;
using neb::kPipeChunkPkts;  // pipe_core.hpp: the staged host pipeline's chunk plan and spans
using neb::kPipeSlots;

struct PipeSlot {
    DevBuf<> d_buf;
    PinnedBuf<neb_desc> h_desc;   // the chunk's rebased descriptors
    DevBuf<neb_desc> d_desc;      // their device copy, which the kernels read
    PinnedBuf<int32_t> h_status;  // mapped: the kernels write it in place
    int32_t* user_status = nullptr;
    uint32_t user_begin = 0, count = 0;
    neb::PipeSpan span;             // arena span of the chunk in flight (count > 0)
    neb::Event in_done;  // the chunk's copies in are done (the kernel waits for it)
    neb::Event k_done;   // its kernel is done (the copies back wait for it)
    neb::Event done;     // its span and statuses are back (the slot is free)
};
struct Pipe {
    neb::Stream h2d, comp, d2h;
    PipeSlot slot[kPipeSlots];
    SchedSpace sched;  // the compute stream's mixed-key workspace

    int ensure(neb_engine* e);         // streams, events and slot buffers: whatever is missing
    hipError_t retire(PipeSlot& s);    // wait for the slot's chunk, hand its statuses to the caller
    void drain();                      // after a failure: nothing queued, no chunk in flight
};

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Host batch path: NEB_HOST_MODE = "zc" (the kernels on the mapped arena, the default) or "dma"
// (hipMemcpyAsync staging); NEB_HOST_STAGED=1 is the older name of "dma". Measured on one MI355X
// (C2 seal+open, 64 Ki x 1300 B): zero-copy 28.4 GiB/s against 23.9 for DMA staging.
enum HostMode { kHostZeroCopy, kHostDma };
HostMode host_mode() {  // NEB_KNOB_HOST_MODE, read per batch, so a process can switch between batches
    return neb::knob(NEB_KNOB_HOST_MODE) == 1 ? kHostDma : kHostZeroCopy;
}

}  // namespace

// Device workspace of the transmit batch (tx.hpp) plus device staging for its host-memory form.
struct TxSpace {
    enum { kWs, kIo };  // dev's buffers: the workspace, neb_tx_seal_batch_host's staging
    neb::HipWorkspace<2> dev;
    uint32_t n_cap = 0, tun_cap = 0, wire_cap = 0;
    neb::TxWs ws{};
    // through a relay (neb_tx_seal_via_batch): the relay tunnels' one key, read back for the outer seal
    PinnedBuf<uint32_t> h_via_key;
    neb::Event via_ev;
    std::mutex mu;
};

// Device workspace of the receive coalescer (coalesce.hpp).
struct CoSpace {
    neb::HipWorkspace<> dev;
    uint32_t n_cap = 0;
    neb::CoWs ws{};
    std::mutex mu;
};

// Device workspace of the TX send plan (send.hpp).
struct SendSpace {
    neb::HipWorkspace<> dev;
    uint32_t n_cap = 0;
    neb::SendWs ws{};
    std::mutex mu;
};

// Device workspace of the RX receive plan (recv.hpp).
struct RecvSpace {
    neb::HipWorkspace<> dev;
    uint32_t n_cap = 0;
    neb::RecvWs ws{};
    std::mutex mu;
};

// Device workspace of the RX batch report (report.hpp).
struct ReportSpace {
    neb::HipWorkspace<> dev;
    uint32_t n_cap = 0;
    neb::ReportWs ws{};
    std::mutex mu;
};

// Per-packet CipherState calls (neb_encrypt_danger / neb_decrypt_danger) and key installs share a
// fixed pool of kPktSlots slots per engine: a stream and pinned, mapped staging the kernel reads
// and writes in place ([desc 64 B | status 64 B | aad | payload + tag]). The box grants a process 4
// hardware queues, so more streams only queue behind each other in the driver. A call takes a free
// slot, or joins one FIFO of waiters and sleeps until a finishing call hands it its slot directly
// (one wake-up per hand-off, nobody spins): the wait of a call is bounded by the calls ahead of
// it, however many threads call. (Round 3 gave every calling OS thread its own slot and stream,
// kept until the engine died: the count grew with the threads cgo ever used, a thread alternating
// over more than 8 engines leaked one per call, and at 64 threads p99 was 100x p50.)
constexpr uint32_t kPktSlots = 4;
struct PktSlot {
    neb::Stream stream;
    PinnedBuf<> h;
};
struct PktWaiter {
    std::condition_variable cv;
    PktSlot* got = nullptr;
};
struct PktPool {
    std::mutex mu;
    PktSlot slot[kPktSlots];
    PktSlot* free_[kPktSlots] = {};
    uint32_t nfree = 0;
    std::deque<PktWaiter*> waiters;
    std::atomic<uint64_t> calls{0}, waits{0};
};
// Per-packet AES-256-GCM calls that arrive while kPktSlots launches are in flight (round 6) ride
// together in one launch: the combiner (comb_core.hpp) over HIP. A call alone is one_packet_solo on a
// slot of the per-packet pool; a batch's buffer is pinned, mapped memory, its launch
// gcm_one_batch_kernel on the pool's streams in turn, its completion handle that stream.
struct HipComb {
    using Buf = PinnedBuf<>;
    using Token = hipStream_t;
    struct Guard {
        DeviceGuard g;
        explicit Guard(HipComb& d);
    };
    neb_engine* e = nullptr;
    bool reserve(Buf& h, size_t bytes);
    int solo(const neb::CombReq& q, int32_t* st);
    bool launch(int open, const neb_desc* desc, int32_t* status, uint8_t* slots, uint32_t n, uint32_t turn, Token& s);
    bool poll(Token&, const int32_t* p);
    bool sync(Token& s);
    void count(uint32_t n);
};
// NEB_PKT_INFLIGHT: launches in flight before calls combine (A/B), default kPktSlots; read once
static uint32_t pkt_inflight() {
    static const uint32_t v = [] {
        const char* s = std::getenv("NEB_PKT_INFLIGHT");
        const int x = s ? std::atoi(s) : (int)kPktSlots;
        return (uint32_t)std::min(std::max(x, 1), 64);
    }();
    return v;
}
using PktComb = neb::CombCore<HipComb>;
struct KeyUse {
    hipStream_t s;
    neb::Event ev;
};

struct neb_engine {
    int device = 0;
    int cu_count = 0;
    neb::Stream stream;
    uint32_t max_keys = 0;
    DevBuf<uint32_t> d_keys;
    std::vector<int> slot_alg;  // 0 = free, -1 = reserved by an install in progress
    // Install id of the key in each slot (0 = none): unique per neb_cipher_create /
    // neb_cipher_create_batch key, shared by the engines of one neb_cipher_create_multi. Batches
    // over several engines check that every shard's engine holds the same install as engine 0.
    std::vector<uint64_t> slot_tag;
    uint64_t key_epoch = 0;  // bumped by every install and destroy (under key_mu)
    std::mutex key_mu;
    uint64_t installs = 0;

    PktPool pkt;  // per-packet calls and key installs
    PktComb comb{pkt_inflight(), kPktSlots};  // per-packet calls combined into one launch

    // Asynchronous batches still queued when a key is destroyed: per key slot, the last
    // single-key batch the engine launched on each stream, and the last mixed-key batch per
    // stream (its keys are only known on the device). neb_cipher_destroy waits for those events
    // only, not for the device.
    std::mutex use_mu;
    std::vector<std::vector<KeyUse>> key_use;
    std::vector<KeyUse> mixed_use;

    std::mutex pipe_mu;
    Pipe pipe;
    // zero-copy host batches: device copies of pageable descriptors / statuses
    DevBuf<neb_desc> zc_desc;
    DevBuf<int32_t> zc_status;

    SchedSpace sched;
    TxSpace tx;
    CoSpace co;
    SendSpace send;
    RecvSpace recv;
    ReportSpace report;

    // The host receive's zero-copy open (neb::RxStaging, window.cpp): a stream and mixed-key
    // workspace of its own, descriptors and statuses staged in pinned memory, one event.
    struct RxSpace {
        std::mutex mu;  // held for the lifetime of a neb::RxStaging
        PinnedBuf<neb_desc> h_desc;
        PinnedBuf<int32_t> h_status;
        DevBuf<neb_desc> d_desc;
        DevBuf<int32_t> d_status;
        neb::Stream stream;
        neb::Event ev;
        SchedSpace sched;
    } rx;

};

struct neb_cipher {
    neb_engine* e;
    uint32_t key_id;
    int alg;
    uint64_t tag;  // neb_engine::slot_tag of the install
};

static thread_local char g_last_error[256] = "";

// neb_set_knob: the environment's values, read once on first use
static std::atomic<int64_t> g_knobs[NEB_KNOB_COUNT];
int64_t neb::knob(int k) {
    static const bool init = [] {
        const char* hm = std::getenv("NEB_HOST_MODE");
        g_knobs[NEB_KNOB_HOST_MODE] = (std::getenv("NEB_HOST_STAGED") || (hm && !std::strcmp(hm, "dma"))) ? 1 : 0;
        const char* sb = std::getenv("NEB_SUB_BINS_FROM");
        g_knobs[NEB_KNOB_SUB_BINS_FROM] = sb ? (int64_t)std::strtoull(sb, nullptr, 10) : (int64_t)neb::kSubBinsFrom;
        const char* mg = std::getenv("NEB_SINGLE_MAX_GRID");
        g_knobs[NEB_KNOB_SINGLE_MAX_GRID] = mg ? std::atoll(mg) : 0;
        g_knobs[NEB_KNOB_RX_STRICT] = std::getenv("NEB_RXDEV_STRICT") ? 1 : 0;
        const char* tb = std::getenv("NEB_TILE_BINS_FROM");
        g_knobs[NEB_KNOB_TILE_BINS_FROM] = tb ? (int64_t)std::strtoull(tb, nullptr, 10) : (int64_t)neb::kTileBinsFrom;
        const char* sb2 = std::getenv("NEB_SMALL_BATCH");
        g_knobs[NEB_KNOB_SMALL_BATCH] = sb2 ? (int64_t)std::strtoull(sb2, nullptr, 10) : (int64_t)neb::kSmallBatchPerWave;
        const char* fg = std::getenv("NEB_FRONT_GROUPS");
        g_knobs[NEB_KNOB_FRONT_GROUPS] = fg ? (int64_t)std::strtoull(fg, nullptr, 10) : (int64_t)neb::kSmallBatchGroups;
        const char* hb = std::getenv("NEB_COALESCE_HASH_BITS");
        g_knobs[NEB_KNOB_COALESCE_HASH_BITS] = hb ? std::atoll(hb) : 32;
        return true;
    }();
    (void)init;
    return g_knobs[k].load(std::memory_order_relaxed);
}
thread_local neb::KernelTiming neb::g_kernel_timing;  // timing.hpp: armed by neb_time_next_kernel
thread_local const void* neb::g_timed_kernel = nullptr;

static void set_error(const char* where, hipError_t err) {
    std::snprintf(g_last_error, sizeof g_last_error, "%s: %s (%d)", where, hipGetErrorString(err), (int)err);
}

#define HIP_TRY(x)                                  \
    do {                                            \
        hipError_t err_ = (x);                      \
        if (err_ != hipSuccess) {                   \
            set_error(#x, err_);                    \
            return NEB_ERR_HIP;                     \
        }                                           \
    } while (0)

// Exclusive use of one slot of e's per-packet pool for the lifetime of the lease (PktPool).
class PktLease {
  public:
    explicit PktLease(PktPool& p) : p_(p) {
        std::unique_lock<std::mutex> lk(p.mu);
        p.calls.fetch_add(1, std::memory_order_relaxed);
        if (p.nfree) {
            s_ = p.free_[--p.nfree];
            return;
        }
        p.waits.fetch_add(1, std::memory_order_relaxed);
        PktWaiter w;
        p.waiters.push_back(&w);
        w.cv.wait(lk, [&] { return w.got != nullptr; });
        s_ = w.got;
    }
    ~PktLease() {
        std::lock_guard<std::mutex> g(p_.mu);
        if (p_.waiters.empty()) {
            p_.free_[p_.nfree++] = s_;
            return;
        }
        PktWaiter* w = p_.waiters.front();  // FIFO: the longest waiter gets the slot
        p_.waiters.pop_front();
        w->got = s_;
        w->cv.notify_one();
    }
    PktLease(const PktLease&) = delete;
    PktLease& operator=(const PktLease&) = delete;
    PktSlot* operator->() const { return s_; }
    // room for `bytes` of staging (the slot is exclusively ours). A per-packet call returns as soon as
    // its kernel has published the status word, so the previous lease's kernel may still be draining
    // on the slot's stream: wait for it before the buffer it writes is freed.
    bool reserve(size_t bytes) {
        const hipError_t err = s_->h.reserve(std::max(kStageMin, align_up(bytes, 1 << 16)), nullptr,
                                             [&] { return hipStreamSynchronize(s_->stream); });
        if (err != hipSuccess) set_error("PktLease::reserve", err);
        return err == hipSuccess;
    }

  private:
    PktPool& p_;
    PktSlot* s_ = nullptr;
};

// The key-use event of (key_hint, s), created on first use (null when that fails); e->use_mu held.
// Events skip the system-scope cache flush (timing-only markers would carry it for nothing).
static hipEvent_t use_event_locked(neb_engine* e, uint32_t key_hint, hipStream_t s) {
    std::vector<KeyUse>& v = key_hint == NEB_KEYS_MIXED ? e->mixed_use : e->key_use[key_hint];
    for (KeyUse& u : v)
        if (u.s == s) return u.ev;
    KeyUse u{s, {}};
    if (u.ev.create(hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) return nullptr;
    v.push_back(std::move(u));
    return v.back().ev;
}
// After an asynchronous batch is enqueued on stream s: remember it for neb_cipher_destroy (the
// key_hint's slot, or every slot for a mixed-key batch).
static void note_use(neb_engine* e, uint32_t key_hint, hipStream_t s) {
    std::lock_guard<std::mutex> g(e->use_mu);
    if (hipEvent_t ev = use_event_locked(e, key_hint, s)) (void)hipEventRecord(ev, s);
}
// The event for a batch to bind to its last kernel (neb_gcm_batch_single's `stop`) instead of
// note_use's marker after it.
static hipEvent_t use_event(neb_engine* e, uint32_t key_hint, hipStream_t s) {
    std::lock_guard<std::mutex> g(e->use_mu);
    return use_event_locked(e, key_hint, s);
}

extern "C" {

NEB_API const char* neb_last_error(void) { return g_last_error; }

NEB_API int neb_time_next_kernel(void* start, void* stop) {
    if ((start == nullptr) != (stop == nullptr)) return NEB_ERR_INVALID;
    neb::g_kernel_timing = {(hipEvent_t)start, (hipEvent_t)stop};
    return NEB_OK;
}

NEB_API int neb_set_knob(int knob, int64_t value) {
    if (knob < 0 || knob >= NEB_KNOB_COUNT) return NEB_ERR_INVALID;
    neb::knob(knob);  // (the environment's values first, so a later first use does not overwrite this)
    g_knobs[knob].store(value, std::memory_order_relaxed);
    return NEB_OK;
}

NEB_API int64_t neb_get_knob(int knob) { return knob < 0 || knob >= NEB_KNOB_COUNT ? -1 : neb::knob(knob); }

NEB_API const char* neb_time_last_kernel(void) {
    static thread_local std::string name;
    if (!neb::g_timed_kernel) return "";
    const char* m = hipKernelNameRefByPtr(neb::g_timed_kernel, nullptr);
    if (!m) return "";
    int st = 0;
    char* d = abi::__cxa_demangle(m, nullptr, nullptr, &st);
    name = st == 0 && d ? d : m;
    std::free(d);
    return name.c_str();
}

#ifndef NEB_BUILD_ID
#define NEB_BUILD_ID "unknown"
#endif
NEB_API const char* neb_build_id(void) { return NEB_BUILD_ID; }

NEB_API const char* neb_strerror(int rc) {
    switch (rc) {
        case NEB_OK: return "ok";
        case NEB_ERR_INVALID: return "invalid argument";
        case NEB_ERR_AUTH: return "cipher: message authentication failed";
        case NEB_ERR_EXHAUSTED: return "message counter exhausted";
        case NEB_ERR_NO_CIPHER: return "no cipher state available to encrypt";
        case NEB_ERR_SHORT_BUFFER: return "output buffer too small";
        case NEB_ERR_HIP: return "HIP runtime error";
        case NEB_ERR_NO_DEVICE: return "no usable gfx950 device";
        case NEB_ERR_NO_KEY_SLOT: return "key table full";
        default: return "unknown error";
    }
}

NEB_API int neb_engine_create(int device, uint32_t max_keys, neb_engine** out) {
    if (!out || max_keys == 0 || max_keys == NEB_KEYS_MIXED) return NEB_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess) {
        set_error("hipGetDeviceCount", err);
        return NEB_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) {
        std::snprintf(g_last_error, sizeof g_last_error, "device %d out of range (%d devices)", device, ndev);
        return NEB_ERR_NO_DEVICE;
    }
    int cus = 0;
    DeviceGuard dg;
    if ((err = hipSetDevice(device)) != hipSuccess ||
        (err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) {
        set_error("hipSetDevice/hipDeviceGetAttribute", err);
        return NEB_ERR_NO_DEVICE;
    }
    // the library carries gfx950 code objects only: a device they do not load on is refused
    if ((err = neb_gcm_probe()) != hipSuccess) {
        set_error("gfx950 code object not loadable on this device", err);
        return NEB_ERR_NO_DEVICE;
    }
    neb_engine* e = new (std::nothrow) neb_engine();
    if (!e) return NEB_ERR_INVALID;
    e->device = device;
    e->comb.dev.e = e;
    e->cu_count = cus;
    e->max_keys = max_keys;
    e->slot_alg.assign(max_keys, 0);
    e->slot_tag.assign(max_keys, 0);
    e->key_use.resize(max_keys);
    bool ok = e->stream.create(hipStreamNonBlocking) == hipSuccess &&
              e->d_keys.reserve((size_t)max_keys * neb::kKeyRecBytes) == hipSuccess &&
              hipMemset(e->d_keys, 0, (size_t)max_keys * neb::kKeyRecBytes) == hipSuccess &&
              hipStreamSynchronize(nullptr) == hipSuccess;  // the null-stream memset, before any stream reads keys
    // The per-packet pool's streams: high priority, which HIP gives a hardware queue of its own each.
    // Streams of the default priority share the process's 4 queues, handed out in the order
    // 1 2 3 4 4 3 2 1 (tools/native/queue_map.cpp under rocprofv3): after the null stream and the
    // engine's stream the pool's 4 landed on 2 queues, and 4 threads' calls ran 2 kernels at a time
    // (round 6 trace, profiles/r6/percall/).
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    for (PktSlot& sl : e->pkt.slot) {
        ok = ok && sl.stream.create_priority(hipStreamNonBlocking, greatest) == hipSuccess &&
             sl.h.reserve(kStageMin) == hipSuccess;
        if (ok) e->pkt.free_[e->pkt.nfree++] = &sl;
    }
    if (!ok) {
        set_error("engine allocation", hipGetLastError());
        neb_engine_destroy(e);
        return NEB_ERR_HIP;
    }
    *out = e;
    return NEB_OK;
}

// Every stream the engine made is waited for, then the members release themselves (hip_owned.hpp;
// each workspace waits for its last batch), here, with the engine's device current.
NEB_API int neb_engine_destroy(neb_engine* e) {
    if (!e) return NEB_ERR_INVALID;
    DeviceGuard dg(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    e->pipe.drain();
    if (e->rx.stream) hipStreamSynchronize(e->rx.stream);
    for (PktSlot& sl : e->pkt.slot)
        if (sl.stream) hipStreamSynchronize(sl.stream);
    delete e;
    return NEB_OK;
}

NEB_API int neb_engine_info(const neb_engine* e, int* device, uint32_t* max_keys, uint32_t* key_record_bytes) {
    if (!e) return NEB_ERR_INVALID;
    if (device) *device = e->device;
    if (max_keys) *max_keys = e->max_keys;
    if (key_record_bytes) *key_record_bytes = neb::kKeyRecBytes;
    return NEB_OK;
}

NEB_API int neb_engine_stats(const neb_engine* e, uint64_t stats[4]) {
    if (!e || !stats) return NEB_ERR_INVALID;
    stats[0] = kPktSlots;
    stats[1] = e->pkt.calls.load(std::memory_order_relaxed);
    stats[2] = e->pkt.waits.load(std::memory_order_relaxed);
    std::lock_guard<std::mutex> g(const_cast<neb_engine*>(e)->key_mu);
    stats[3] = e->installs;
    return NEB_OK;
}

NEB_API const char* neb_cipher_name(int alg) {
    return alg == NEB_ALG_AESGCM ? "AESGCM" : alg == NEB_ALG_CHACHAPOLY ? "ChaChaPoly" : nullptr;
}

static std::atomic<uint64_t> g_key_tag{1};

// Reserve the n lowest free slots of e (caller holds e->key_mu); false if fewer are free.
static bool reserve_slots(neb_engine* e, uint32_t n, uint32_t* slots) {
    uint32_t k = 0;
    for (uint32_t s = 0; s < e->max_keys && k < n; s++)
        if (e->slot_alg[s] == 0) slots[k++] = s;
    if (k < n) return false;
    for (uint32_t i = 0; i < n; i++) e->slot_alg[slots[i]] = -1;
    return true;
}

// Key install of n keys into the reserved slots slots[0..n), one launch: the keys and slot numbers go
// through one slot of the per-packet pool (pinned, mapped: the setup kernel reads them there), each
// workgroup clears its record and installs one key, and the staged key bytes are wiped afterwards.
// On failure the records are cleared again, so no slot is left holding a half-written record
// whose algorithm tag a batch could accept.
static int install_records(neb_engine* e, int alg, const uint8_t* keys, const uint32_t* slots, uint32_t n) {
    DeviceGuard dg(e->device);
    PktLease sl(e->pkt);
    const size_t kb = align_up((size_t)n * 32u, 64);
    if (!sl.reserve(kb + (size_t)n * 4u)) return NEB_ERR_HIP;
    std::memcpy(sl->h, keys, (size_t)n * 32u);
    std::memcpy(sl->h + kb, slots, (size_t)n * 4u);
    hipError_t err = alg == NEB_ALG_AESGCM
                         ? neb_gcm_key_setup(sl->h, (const uint32_t*)(sl->h + kb), n, e->d_keys, sl->stream)
                         : neb_chacha_key_setup(sl->h, (const uint32_t*)(sl->h + kb), n, e->d_keys, sl->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(sl->stream);
    std::memset(sl->h, 0, (size_t)n * 32u);
    if (err != hipSuccess) {
        set_error("key setup", err);
        for (uint32_t i = 0; i < n; i++)
            (void)hipMemsetAsync(e->d_keys + (size_t)slots[i] * neb::kKeyRecDwords, 0, neb::kKeyRecBytes, sl->stream);
        (void)hipStreamSynchronize(sl->stream);
        return NEB_ERR_HIP;
    }
    return NEB_OK;
}

// Publish (rc == NEB_OK) or release the reserved slots; caller holds e->key_mu.
static void commit_slots(neb_engine* e, int alg, const uint32_t* slots, const uint64_t* tags, uint32_t n, bool ok) {
    for (uint32_t i = 0; i < n; i++) {
        e->slot_alg[slots[i]] = ok ? alg : 0;
        e->slot_tag[slots[i]] = ok ? tags[i] : 0;
    }
    if (ok) {
        e->installs += n;
        e->key_epoch++;
    }
}

static bool valid_alg(int alg) { return alg == NEB_ALG_AESGCM || alg == NEB_ALG_CHACHAPOLY; }

NEB_API int neb_cipher_create_batch(neb_engine* e, int alg, const uint8_t* keys, uint32_t n, neb_cipher** out) {
    if (!e || !out || !valid_alg(alg) || (n && !keys)) return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    for (uint32_t i = 0; i < n; i++) out[i] = nullptr;
    std::vector<uint32_t> slots(n);
    std::vector<uint64_t> tags(n);
    std::vector<neb_cipher*> cs(n, nullptr);
    for (uint32_t i = 0; i < n; i++) {
        cs[i] = new (std::nothrow) neb_cipher{e, 0, alg, 0};
        if (!cs[i]) {
            for (neb_cipher* c : cs) delete c;
            return NEB_ERR_INVALID;
        }
    }
    {
        std::lock_guard<std::mutex> g(e->key_mu);
        if (!reserve_slots(e, n, slots.data())) {
            for (neb_cipher* c : cs) delete c;
            return NEB_ERR_NO_KEY_SLOT;
        }
    }
    const int rc = install_records(e, alg, keys, slots.data(), n);
    const uint64_t t0 = g_key_tag.fetch_add(n);
    for (uint32_t i = 0; i < n; i++) tags[i] = t0 + i;
    std::lock_guard<std::mutex> g(e->key_mu);
    commit_slots(e, alg, slots.data(), tags.data(), n, rc == NEB_OK);
    for (uint32_t i = 0; i < n; i++) {
        if (rc != NEB_OK) {
            delete cs[i];
            continue;
        }
        cs[i]->key_id = slots[i];
        cs[i]->tag = tags[i];
        out[i] = cs[i];
    }
    return rc;
}

NEB_API int neb_cipher_create(neb_engine* e, int alg, const uint8_t key[32], neb_cipher** out) {
    if (!e || !key || !out || !valid_alg(alg)) return NEB_ERR_INVALID;
    *out = nullptr;
    return neb_cipher_create_batch(e, alg, key, 1, out);
}

NEB_API int neb_cipher_create_multi(neb_engine* const* engines, uint32_t m, int alg, const uint8_t key[32],
                                    neb_cipher** out) {
    if (!engines || m == 0 || !key || !out || !valid_alg(alg)) return NEB_ERR_INVALID;
    std::vector<neb_engine*> es(engines, engines + m);
    for (uint32_t k = 0; k < m; k++) {
        out[k] = nullptr;
        if (!es[k]) return NEB_ERR_INVALID;
    }
    std::vector<neb_engine*> order = es;
    std::sort(order.begin(), order.end());
    if (std::adjacent_find(order.begin(), order.end()) != order.end()) return NEB_ERR_INVALID;  // an engine twice
    std::vector<neb_cipher*> cs(m, nullptr);
    for (uint32_t k = 0; k < m; k++)
        if (!(cs[k] = new (std::nothrow) neb_cipher{es[k], 0, alg, 0})) {
            for (neb_cipher* c : cs) delete c;
            return NEB_ERR_INVALID;
        }
    // the lowest slot free on every engine, reserved on all of them at once (engines locked in
    // address order, so two concurrent multi-installs cannot deadlock)
    uint32_t slot = 0;
    {
        for (neb_engine* e : order) e->key_mu.lock();
        uint32_t lim = ~0u;
        for (neb_engine* e : es) lim = std::min(lim, e->max_keys);
        bool found = false;
        for (; slot < lim && !found; slot++) {
            found = true;
            for (neb_engine* e : es) found = found && e->slot_alg[slot] == 0;
            if (found) break;
        }
        if (found)
            for (neb_engine* e : es) e->slot_alg[slot] = -1;
        for (neb_engine* e : order) e->key_mu.unlock();
        if (!found) {
            for (neb_cipher* c : cs) delete c;
            return NEB_ERR_NO_KEY_SLOT;
        }
    }
    int rc = NEB_OK;
    std::vector<int> done(m, 0);
    for (uint32_t k = 0; k < m && rc == NEB_OK; k++) {
        rc = install_records(es[k], alg, key, &slot, 1);
        done[k] = rc == NEB_OK;
    }
    const uint64_t tag = g_key_tag.fetch_add(1);
    for (uint32_t k = 0; k < m; k++) {
        neb_engine* e = es[k];
        if (rc != NEB_OK && done[k]) {  // roll back the engines that had installed it
            DeviceGuard dg(e->device);
            PktLease sl(e->pkt);
            (void)hipMemsetAsync(e->d_keys + (size_t)slot * neb::kKeyRecDwords, 0, neb::kKeyRecBytes, sl->stream);
            (void)hipStreamSynchronize(sl->stream);
        }
        std::lock_guard<std::mutex> g(e->key_mu);
        commit_slots(e, alg, &slot, &tag, 1, rc == NEB_OK);
        if (rc == NEB_OK) {
            cs[k]->key_id = slot;
            cs[k]->tag = tag;
            out[k] = cs[k];
        } else {
            delete cs[k];
        }
    }
    return rc;
}

NEB_API int neb_cipher_destroy(neb_cipher* c) {
    if (!c) return NEB_ERR_INVALID;
    neb_engine* e = c->e;
    const uint32_t slot = c->key_id;
    DeviceGuard dg(e->device);
    // Asynchronous batches the engine enqueued that may read this record: the last single-key
    // batch with this key on each stream, the last mixed-key batch on each stream (note_use), and
    // the mixed-key AES-GCM batches of the engine's scheduler workspace. Those have no key-use
    // marker of their own (it cost ≈ 5 µs per batch): the workspace's `done` event is recorded
    // after each and every later user waits for it, so the destroy waits for the workspace's
    // latest batch — which may be another tunnel's batch enqueued after the last one that used
    // this key, so a teardown can wait behind unrelated mixed-key traffic on this engine (at most
    // the batches enqueued before the destroy; never the whole device).
    // The caller stops enqueuing with a key before destroying it.
    std::vector<hipEvent_t> wait;
    {
        std::lock_guard<std::mutex> g(e->use_mu);
        for (KeyUse& u : e->key_use[slot]) wait.push_back(u.ev);
        for (KeyUse& u : e->mixed_use) wait.push_back(u.ev);
    }
    {
        std::lock_guard<std::mutex> g(e->sched.mu);
        if (e->sched.dev.event()) wait.push_back(e->sched.dev.event());
    }
    for (hipEvent_t ev : wait) (void)hipEventSynchronize(ev);
    int rc = NEB_OK;
    {
        PktLease sl(e->pkt);
        if (hipMemsetAsync(e->d_keys + (size_t)slot * neb::kKeyRecDwords, 0, neb::kKeyRecBytes, sl->stream) !=
                hipSuccess ||
            hipStreamSynchronize(sl->stream) != hipSuccess)
            rc = NEB_ERR_HIP;
    }
    {
        std::lock_guard<std::mutex> g(e->use_mu);
        e->key_use[slot].clear();
    }
    {
        std::lock_guard<std::mutex> g(e->key_mu);
        e->slot_alg[slot] = 0;
        e->slot_tag[slot] = 0;
        e->key_epoch++;
    }
    delete c;
    return rc;
}

NEB_API uint32_t neb_cipher_key_id(const neb_cipher* c) { return c ? c->key_id : NEB_KEYS_MIXED; }
NEB_API int neb_cipher_alg(const neb_cipher* c) { return c ? c->alg : 0; }
NEB_API int neb_overhead(const neb_cipher* c) { return c ? NEB_OVERHEAD : 0; }

static void fill_nonce(int alg, uint64_t n, uint8_t* nb) {
    if (!nb) return;
    nb[0] = nb[1] = nb[2] = nb[3] = 0;
    for (int i = 0; i < 8; i++) nb[4 + i] = alg == NEB_ALG_AESGCM ? (uint8_t)(n >> (56 - 8 * i)) : (uint8_t)(n >> (8 * i));
}

// Size the scheduler workspace for n packets (caller holds sched.mu). The counters are cleared on
// the batch's own stream: a plain hipMemset runs on the null stream, which a non-blocking stream
// does not wait for, and may still be running when the binning starts (measured: the first batches
// of a queue lost most of their packets' statuses to it).
static hipError_t sched_reserve(neb_engine* e, SchedSpace& sp, uint32_t n, hipStream_t s) {
    // the tile binning's arrays (sched.hpp), only for workspaces that see batches that large: a
    // queue's small batches keep the atomic histogram and need none
    const bool tiles = (int64_t)n >= neb::knob(NEB_KNOB_TILE_BINS_FROM) || sp.ws.tcnt;
    const bool fits = n <= sp.n_cap && sp.dev.mem() && (!tiles || sp.ws.tcnt);
    if (fits && !sp.dirty) return hipSuccess;
    if (fits) {  // the bins are cleared as they are consumed, except after a failure
        hipError_t err = sp.dev.sync();
        if (err == hipSuccess)
            err = hipMemsetAsync(sp.ws.counters, 0, (neb::kSchedCounters + (size_t)neb::kSubBins * neb::sched_nbins(e->max_keys)) * 4u, s);
        if (err == hipSuccess) sp.dirty = false;
        return err;
    }
    const uint32_t cap = std::max<uint32_t>(n, 1u << 16);
    const uint32_t nb = neb::sched_nbins(e->max_keys);
    const uint32_t mc = neb::sched_max_chunks(cap, e->max_keys);
    const size_t b_counters = align_up((neb::kSchedCounters + (size_t)neb::kSubBins * nb) * 4u, 256);
    const size_t b_base = align_up((size_t)neb::kSubBins * nb * 4u, 256);
    const size_t b_idx = align_up((size_t)cap * 4u, 256), b_chunks = align_up((size_t)neb::kBuckets * mc * 16u, 256);
    const size_t b_tcnt = tiles ? align_up((size_t)neb::kTileMax * neb::sched_tile_words(nb) * 4u, 256) : 0;
    const size_t b_tpre = tiles ? align_up((size_t)neb::kTileMax * nb * 4u, 256) : 0;
    const size_t bytes = b_counters + b_base + 3 * b_idx + b_chunks + b_tcnt + b_tpre;
    sp.n_cap = 0;
    bool grew = false;
    hipError_t err = sp.dev.reserve(bytes, &grew);
    if (err == hipSuccess && !grew) err = sp.dev.sync();  // (as many bytes, laid out again: as after growing)
    if (err != hipSuccess) return err;
    uint8_t* m = sp.dev.mem();
    auto take = [&m](size_t b) { return (m += b) - b; };  // the next b bytes
    sp.ws.counters = (uint32_t*)take(b_counters);
    sp.ws.hist = sp.ws.counters + neb::kSchedCounters;
    sp.ws.base = (uint32_t*)take(b_base);
    sp.ws.binof = (uint32_t*)take(b_idx);
    sp.ws.binpos = (uint32_t*)take(b_idx);
    sp.ws.sorted = (uint32_t*)take(b_idx);
    sp.ws.chunks = (uint4*)take(b_chunks);
    sp.ws.tcnt = tiles ? (uint32_t*)take(b_tcnt) : nullptr;
    sp.ws.tpre = tiles ? (uint32_t*)take(b_tpre) : nullptr;
    sp.ws.max_chunks = mc;
    sp.n_cap = cap;
    err = hipMemsetAsync(sp.ws.counters, 0, b_counters, s);  // once: the binning clears its counts as it uses them
    if (err == hipSuccess) sp.dirty = false;
    return err;
}

// Groups per front chunk at most (sched_groups' own: up to 8) for a batch of n packets: below
// NEB_KNOB_SMALL_BATCH packets per resident wave of the chunk kernel (16 per CU) the front chunks hold
// NEB_KNOB_FRONT_GROUPS groups at most (sched.hpp kSmallBatchPerWave).
static uint32_t front_groups(const neb_engine* e, uint32_t n) {
    const int64_t below = neb::knob(NEB_KNOB_SMALL_BATCH), cap = neb::knob(NEB_KNOB_FRONT_GROUPS);
    const uint64_t waves = (uint64_t)std::max(e->cu_count, 1) * 16u;
    return below > 0 && cap > 0 && (uint64_t)n < (uint64_t)below * waves ? (uint32_t)std::min<int64_t>(cap, 8) : 8u;
}

// One seal or open of a batch (neb::BatchLaunch, engine_internal.hpp). b.d_n: a batch whose size is
// only known on the device, e.g. the segments of a TX batch. b.rx: only packets with rx[i] != 0 are
// opened, the others keep the statuses the receive's plan wrote (window.cpp, rxwin.hip).
// b.prebinned: the mixed-key binning of this batch is already in b.sched (neb_rx_sched_begin,
// ordered before b.stream).
static hipError_t launch_batch(neb_engine* e, const BatchLaunch& b) {
    hipStream_t s = b.stream;
    if (b.alg == NEB_ALG_AESGCM) {
        if (b.key_hint != NEB_KEYS_MIXED)
            return neb_gcm_batch_single(b.open, b.desc, b.n, b.arena, e->d_keys, e->max_keys, b.key_hint, b.status,
                                        b.d_n, e->cu_count, s, b.hdr_from_dst, b.stop, b.rx);
        // mixed keys: regroup into single-key, similar-size chunks on the device, then seal/open
        SchedSpace& sp = b.sched ? *b.sched : e->sched;
        std::lock_guard<std::mutex> g(sp.mu);
        hipError_t err = hipSuccess;
        if (!b.prebinned) {
            err = sched_reserve(e, sp, b.n, s);
            if (err == hipSuccess) err = sp.dev.begin(s);  // after the previous batch on it
            neb::SchedWs ws = sp.ws;
            ws.max_groups = front_groups(e, b.n);
            if (err == hipSuccess) err = neb_sched_build(b.desc, b.n, b.d_n, e->max_keys, 4u, &ws, s);
        }
        if (err == hipSuccess)  // the workspace's event bound to the chunk kernel's dispatch: no marker packet between batches
            err = neb_gcm_batch_chunked(b.open, b.desc, b.n, b.arena, e->d_keys, e->max_keys, b.status, sp.ws.sorted,
                                        sp.ws.chunks, sp.ws.counters, sp.ws.max_chunks, e->cu_count,
                                        s, b.hdr_from_dst, sp.dev.event(),
                                        b.prebinned ? nullptr : b.rx);  // (prebinned: refused packets unlisted)
        if (err == hipSuccess) {
            sp.dev.end_bound(s);
        } else {
            // binning passes of this batch may already be queued on s: let them finish before the
            // next batch clears the counters (sched_reserve's dirty path waits on the event only)
            (void)hipStreamSynchronize(s);
            sp.dirty = true;
        }
        return err;
    }
    return neb_chacha_batch(b.open, b.desc, b.n, b.arena, e->d_keys, e->max_keys, b.key_hint, b.status, b.d_n,
                            e->cu_count, s, b.hdr_from_dst, b.stop, b.rx);
}

// Poll a per-packet call's status word in pinned host memory (-1 until the kernel publishes it) for up
// to kPollUs; false when it has not come by then (the caller waits for the stream instead). A
// pinned-memory poll sees the kernel's last store within about a microsecond of it; the stream
// synchronize took ≈ 26 µs of the ≈ 36 µs call at 4 threads in round 4.
constexpr int kPollUs = 2000;
static bool poll_status(const int32_t* p, int32_t* st, int us = kPollUs) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t i = 0;; i++) {
        const int32_t v = __atomic_load_n(p, __ATOMIC_ACQUIRE);
        if (v != -1) {
            *st = v;
            return true;
        }
        __builtin_ia32_pause();
        if ((i & 255u) == 255u &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(us))
            return false;
    }
}

using neb::copy_result;  // comb_core.hpp

// One packet through the device, on a slot of the engine's per-packet pool (PktPool): the packet is
// copied into the slot's pinned, mapped buffer ([desc | status | aad | payload (+tag)]), the batch
// kernel seals or opens it there in place (zero-copy: no DMA either way) and the result is copied
// out. Up to kPktSlots calls run side by side; later ones wait their turn in FIFO order.
static int one_packet_solo(neb_engine* e, const neb::CombReq& q, int32_t* st_out) {
    const int alg = q.alg, open = q.open;
    const uint32_t key_id = q.key_id;
    const uint8_t *ad = q.ad, *in = q.in;
    const size_t ad_len = q.ad_len, in_len = q.in_len, pay_len = q.pay_len;
    const uint64_t n = q.n;
    uint8_t* dst = q.dst;
    const size_t o_desc = 0, o_status = 64, o_aad = 128;
    const size_t o_pay = align_up(o_aad + ad_len, 16);
    const size_t total = o_pay + pay_len + 16;
    DeviceGuard dg(e->device);
    PktLease sl(e->pkt);
    if (!sl.reserve(total)) return NEB_ERR_HIP;
    uint8_t* h = sl->h;
    // The packet's bytes travel in the kernel's arguments and only the result comes back through
    // the slot (aes_gcm.hip gcm_one_kernel, chacha_poly.hip chacha_one_kernel).
    *(int32_t*)(h + o_status) = -1;
    auto* fn = alg == NEB_ALG_AESGCM ? neb_gcm_one : neb_chacha_one;
    hipError_t err = fn(open, ad, (uint32_t)ad_len, in, (uint32_t)in_len, (uint32_t)pay_len, n, h + o_pay,
                        (int32_t*)(h + o_status), e->d_keys, e->max_keys, key_id, sl->stream);
    if (err == hipSuccess) {
        // the kernel publishes the status last, behind a system-scope release of the result
        // (device_common.hpp one_publish_status): poll it, and wait for the stream only if it
        // does not come (a fault reports there)
        int32_t st = -1;
        if (!poll_status(reinterpret_cast<const int32_t*>(h + o_status), &st)) {
            err = hipStreamSynchronize(sl->stream);
            if (err != hipSuccess) {
                set_error("one_packet", err);
                return NEB_ERR_HIP;
            }
            st = __atomic_load_n(reinterpret_cast<const int32_t*>(h + o_status), __ATOMIC_ACQUIRE);
        }
        *st_out = st;
        copy_result(open, st, dst, h + o_pay, pay_len);
        return NEB_OK;
    }
    if (err != hipErrorInvalidValue) {
        set_error("one_packet", err);
        return NEB_ERR_HIP;
    }
    (void)hipGetLastError();
    // too large for the kernel arguments: one descriptor through the batch path
    neb_desc d{};
    d.src_off = o_pay - o_aad;
    d.dst_off = o_pay - o_aad;
    d.aad_off = 0;
    d.counter = n;
    d.len = (uint32_t)pay_len;
    d.aad_len = (uint32_t)ad_len;
    d.key_id = key_id;
    std::memcpy(h + o_desc, &d, sizeof d);
    *(int32_t*)(h + o_status) = -1;
    if (ad_len) std::memcpy(h + o_aad, ad, ad_len);
    if (in_len) std::memcpy(h + o_pay, in, in_len);
    err = launch_batch(e, {.alg = alg, .open = open, .desc = (const neb_desc*)(h + o_desc), .n = 1, .arena = h + o_aad,
                           .status = (int32_t*)(h + o_status), .key_hint = key_id, .stream = sl->stream});
    if (err == hipSuccess) err = hipStreamSynchronize(sl->stream);
    if (err != hipSuccess) {
        set_error("one_packet", err);
        return NEB_ERR_HIP;
    }
    std::memcpy(st_out, h + o_status, 4);
    copy_result(open, *st_out, dst, h + o_pay, pay_len);
    return NEB_OK;
}

// The combiner's device (comb_core.hpp) on HIP.
HipComb::Guard::Guard(HipComb& d) : g(d.e->device) {}
bool HipComb::reserve(Buf& h, size_t bytes) {
    if (h.reserve(bytes) == hipSuccess) return true;
    set_error("pinned memory (per-packet batch)", hipErrorOutOfMemory);
    return false;
}
int HipComb::solo(const neb::CombReq& q, int32_t* st) { return one_packet_solo(e, q, st); }
bool HipComb::launch(int open, const neb_desc* desc, int32_t* status, uint8_t* slots, uint32_t n, uint32_t turn,
                     Token& s) {
    s = e->pkt.slot[turn % kPktSlots].stream;  // the per-packet pool's streams carry the combined launches in turn
    const hipError_t err = neb_gcm_one_batch(open, desc, status, slots, n, e->d_keys, e->max_keys, s);
    if (err != hipSuccess) set_error("per-packet batch launch", err);
    return err == hipSuccess;
}
bool HipComb::poll(Token&, const int32_t* p) {
    int32_t v;
    return poll_status(p, &v);
}
bool HipComb::sync(Token& s) {
    const hipError_t err = hipStreamSynchronize(s);
    if (err != hipSuccess) set_error("per-packet batch launch", err);
    return err == hipSuccess;
}
void HipComb::count(uint32_t n) { e->pkt.calls.fetch_add(n, std::memory_order_relaxed); }  // (neb_engine_stats)

// A per-packet call through the engine's combiner (PktComb, comb_core.hpp): alone while a launch
// slot is free (one_packet_solo: the packet in the kernel arguments), else as a request of the
// batch the next completed launch frees a slot for. AES-256-GCM only (the ChaCha20-Poly1305 batch
// kernel's statuses carry no release of the payload before them, so its calls stay alone).
static int one_packet(neb_cipher* c, int open, const uint8_t* ad, size_t ad_len, const uint8_t* in, size_t in_len,
                      size_t pay_len, uint64_t n, uint8_t* dst, int32_t* st_out) {
    neb::CombReq q;
    q.alg = c->alg;
    q.open = open;
    q.key_id = c->key_id;
    q.n = n;
    q.ad = ad;
    q.ad_len = ad_len;
    q.in = in;
    q.in_len = in_len;
    q.pay_len = pay_len;
    q.dst = dst;
    return c->e->comb.call(q, st_out);
}

// Per-packet calls combined into shared launches: {launches of combined batches, calls they carried}
NEB_API int neb_engine_pkt_combined(const neb_engine* e, uint64_t out[2]) {
    if (!e || !out) return NEB_ERR_INVALID;
    e->comb.counters(out);
    return NEB_OK;
}

// For tests: req[0..n) as one combined launch, request r in slot r (CombCore::run).
NEB_API int neb_engine_pkt_launch(neb_engine* e, int open, const neb_pkt_req* req, uint32_t n, int32_t* status) {
    if (!e || n > neb::kCombMax || (n && (!req || !status))) return NEB_ERR_INVALID;
    neb::CombReq q[neb::kCombMax];
    for (uint32_t r = 0; r < n; r++) {
        const neb_pkt_req& p = req[r];
        if ((!p.ad && p.ad_len) || (!p.in && p.in_len) || !p.out || (open && p.in_len < NEB_OVERHEAD)) return NEB_ERR_INVALID;
        q[r].alg = NEB_ALG_AESGCM;
        q[r].open = open ? 1 : 0;
        q[r].key_id = p.key_id;
        q[r].n = p.counter;
        q[r].ad = p.ad;
        q[r].ad_len = p.ad_len;
        q[r].in = p.in;
        q[r].in_len = p.in_len;
        q[r].pay_len = open ? p.in_len - NEB_OVERHEAD : p.in_len;
        q[r].dst = p.out;
    }
    return e->comb.run(open ? 1 : 0, q, n, status);
}

NEB_API int neb_encrypt_danger(neb_cipher* c, uint8_t* out, size_t out_len, size_t out_cap, const uint8_t* ad,
                               size_t ad_len, const uint8_t* pt, size_t pt_len, uint64_t n, uint8_t* nb,
                               size_t* ret_len) {
    if (ret_len) *ret_len = 0;
    if (!c) return NEB_ERR_NO_CIPHER;  // aesgcm.go:25-27
    if (n >= NEB_REJECT_AFTER_MESSAGES) return NEB_ERR_EXHAUSTED;  // aesgcm.go:28-30
    if ((!out && out_cap) || (!ad && ad_len) || (!pt && pt_len) || pt_len > 0xFFFFFFF0u || ad_len > 0xFFFFFFF0u)
        return NEB_ERR_INVALID;
    if (out_cap < out_len || out_cap - out_len < pt_len + NEB_OVERHEAD) return NEB_ERR_SHORT_BUFFER;
    fill_nonce(c->alg, n, nb);
    int32_t st = -1;
    int rc = one_packet(c, 0, ad, ad_len, pt, pt_len, pt_len, n, out + out_len, &st);
    if (rc != NEB_OK) return rc;
    if (st != NEB_STATUS_OK) return st == NEB_STATUS_EXHAUSTED ? NEB_ERR_EXHAUSTED : NEB_ERR_INVALID;
    if (ret_len) *ret_len = out_len + pt_len + NEB_OVERHEAD;
    return NEB_OK;
}

NEB_API int neb_decrypt_danger(neb_cipher* c, uint8_t* out, size_t out_len, size_t out_cap, const uint8_t* ad,
                               size_t ad_len, const uint8_t* ct, size_t ct_len, uint64_t n, uint8_t* nb,
                               size_t* ret_len) {
    if (ret_len) *ret_len = 0;
    if (!c) return NEB_OK;  // aesgcm.go:40-42: ([]byte{}, nil)
    if ((!ad && ad_len) || (!ct && ct_len) || ct_len > 0xFFFFFFF0u || ad_len > 0xFFFFFFF0u) return NEB_ERR_INVALID;
    fill_nonce(c->alg, n, nb);
    if (ct_len < NEB_OVERHEAD) return NEB_ERR_AUTH;  // Open: ciphertext shorter than the tag
    const size_t pt_len = ct_len - NEB_OVERHEAD;
    if ((!out && out_cap) || out_cap < out_len || out_cap - out_len < pt_len) return NEB_ERR_SHORT_BUFFER;
    int32_t st = -1;
    int rc = one_packet(c, 1, ad, ad_len, ct, ct_len, pt_len, n, out + out_len, &st);
    if (rc != NEB_OK) return rc;
    if (st == NEB_STATUS_AUTH_FAILED) return NEB_ERR_AUTH;  // plaintext region already zeroed
    if (st != NEB_STATUS_OK) return NEB_ERR_INVALID;
    if (ret_len) *ret_len = out_len + pt_len;
    return NEB_OK;
}

static int check_batch(neb_engine* e, int alg, uint32_t key_hint) {
    if (!e || (alg != NEB_ALG_AESGCM && alg != NEB_ALG_CHACHAPOLY)) return NEB_ERR_INVALID;
    if (key_hint != NEB_KEYS_MIXED) {
        std::lock_guard<std::mutex> g(e->key_mu);
        if (key_hint >= e->max_keys || e->slot_alg[key_hint] != alg) return NEB_ERR_INVALID;
    }
    return NEB_OK;
}

static int batch_device(neb_engine* e, int alg, int open, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                        int32_t* d_status, uint32_t key_hint, void* stream) {
    int rc = check_batch(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (n == 0) return NEB_OK;
    if (!d_desc || !d_arena || !d_status) return NEB_ERR_INVALID;
    DeviceGuard dg(e->device);
    hipStream_t s = (hipStream_t)stream;  // NULL = the HIP default stream, as for any HIP launch
    // A batch binds its key-use event to its last kernel (no marker packet after it: each marker
    // between two batches cost ≈ 5 µs, C3 +3.5-5%, profiles/r3_ab/use_events.log). A mixed-key
    // AES-GCM batch runs through the engine's scheduler workspace, whose `done` event is bound to
    // its chunk kernel the same way and orders every later user of the workspace after it;
    // neb_cipher_destroy waits on that event, so it needs no key-use event of its own.
    const bool sched = alg == NEB_ALG_AESGCM && key_hint == NEB_KEYS_MIXED;
    hipEvent_t stop = sched ? nullptr : use_event(e, key_hint, s);
    hipError_t err = launch_batch(e, {.alg = alg, .open = open, .desc = d_desc, .n = n, .arena = d_arena,
                                      .status = d_status, .key_hint = key_hint, .stream = s, .stop = stop});
    if (err != hipSuccess) {
        set_error("batch launch", err);
        return NEB_ERR_HIP;
    }
    if (!sched && !stop) note_use(e, key_hint, s);  // no event could be created: a marker
    return NEB_OK;
}

NEB_API int neb_seal_batch(neb_engine* e, int alg, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                           int32_t* d_status, uint32_t key_hint, void* stream) {
    return batch_device(e, alg, 0, d_desc, n, d_arena, d_status, key_hint, stream);
}

NEB_API int neb_open_batch(neb_engine* e, int alg, const neb_desc* d_desc, uint32_t n, uint8_t* d_arena,
                           int32_t* d_status, uint32_t key_hint, void* stream) {
    return batch_device(e, alg, 1, d_desc, n, d_arena, d_status, key_hint, stream);
}

// ---- for the device batched receive (window.cpp, rxwin.hip); internal ------------------------

int neb_engine_device_of(const neb_engine* e) { return e->device; }
int neb_check_batch_args(neb_engine* e, int alg, uint32_t key_hint) { return check_batch(e, alg, key_hint); }

// The launch of window.cpp (the device receive's opens, the relay forwarding's seal) and queue.cpp
// (one staged batch, zero-copy on pinned memory, on the queue's stream); the caller has made the
// engine's device current.
int neb_launch(neb_engine* e, const BatchLaunch& b) {
    if (b.n == 0) return NEB_OK;
    hipError_t err = launch_batch(e, b);
    if (err != hipSuccess) {
        set_error("batch launch", err);
        return NEB_ERR_HIP;
    }
    if (b.note_use) note_use(e, b.key_hint, b.stream);
    return NEB_OK;
}

// Relay forwarding (window.cpp, relay.hip): the key table its plan checks the tunnels' keys against.
void neb_engine_key_table(const neb_engine* e, const uint32_t** d_keys, uint32_t* max_keys) {
    *d_keys = e->d_keys;
    *max_keys = e->max_keys;
}

// A scheduler workspace of its own for each of the submission queue's batches (queue.cpp) and for
// the device receive (window.cpp).
SchedSpace* neb_sched_space_new() { return new (std::nothrow) SchedSpace; }
void neb_sched_space_free(SchedSpace* sp) { delete sp; }  // ~DevWorkspace waits for the last batch on it

// The device receive (window.cpp): its mixed-key AES-GCM open is binned by extra workgroups of the
// receive's own plan launches (rxwin.hpp RxBin) into the receive's scheduler workspace `sched`,
// which this sizes for n packets and orders after its last open; the open then runs with it
// (BatchLaunch::prebinned). neb_rx_sched_abort after a failed plan (the counters are
// then in an unknown state: the next batch clears them).
int neb_rx_sched_begin(neb_engine* e, uint32_t n, SchedSpace* sched, hipStream_t s, neb::SchedWs* ws,
                       uint32_t* max_keys) {
    SchedSpace& sp = *sched;
    std::lock_guard<std::mutex> g(sp.mu);
    hipError_t err = sched_reserve(e, sp, n, s);
    if (err == hipSuccess) err = sp.dev.begin(s);  // after the last open's reads
    if (err != hipSuccess) {
        sp.dirty = true;
        set_error("rx binning", err);
        return NEB_ERR_HIP;
    }
    *ws = sp.ws;
    ws->max_groups = front_groups(e, n);
    *max_keys = e->max_keys;
    return NEB_OK;
}
void neb_rx_sched_abort(SchedSpace* sched) {
    std::lock_guard<std::mutex> g(sched->mu);
    sched->dirty = true;
}
int neb_key_alg(neb_engine* e, uint32_t key) {
    std::lock_guard<std::mutex> g(e->key_mu);
    return key < e->max_keys ? e->slot_alg[key] : 0;
}

// True if p is pinned host memory the device addresses at the same pointer (hipHostMalloc).
static bool host_mapped(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost && a.devicePointer == p;
}
bool neb_host_mapped(const void* p) { return host_mapped(p); }  // queue.cpp

// Zero-copy host batch: the arena is pinned and mapped, so the kernels load and store it across
// PCIe themselves (loads = the H2D direction, stores = D2H, both at once) with no staging copies.
// Pageable descriptors / statuses go through device buffers. Every descriptor is bounds-checked
// on the host first: a kernel access outside the mapping would fault the GPU.
static int batch_host_zero_copy(neb_engine* e, int alg, int open, const neb_desc* desc, uint32_t n,
                                uint8_t* arena, size_t arena_len, int32_t* status, uint32_t key_hint) {
    const bool desc_mapped = host_mapped(desc), status_mapped = host_mapped(status);
    if (!desc_mapped || !status_mapped) {
        auto idle = [&] { return hipStreamSynchronize(e->stream); };
        HIP_TRY(e->zc_desc.reserve((size_t)n * sizeof(neb_desc), nullptr, idle));
        HIP_TRY(e->zc_status.reserve((size_t)n * sizeof(int32_t), nullptr, idle));
    }
    const neb_desc* d_desc = desc;
    int32_t* d_status = status;
    if (!desc_mapped) {
        HIP_TRY(hipMemcpyAsync(e->zc_desc, desc, (size_t)n * sizeof(neb_desc), hipMemcpyHostToDevice, e->stream));
        d_desc = e->zc_desc;
    }
    if (!status_mapped) d_status = e->zc_status;
    HIP_TRY(launch_batch(e, {.alg = alg, .open = open, .desc = d_desc, .n = n, .arena = arena, .status = d_status,
                             .key_hint = key_hint, .stream = e->stream}));
    if (!status_mapped)
        HIP_TRY(hipMemcpyAsync(status, d_status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return NEB_OK;
}

// ---- the staged host pipeline (pipe_core.hpp) -------------------------------------------------

// Each of the pipeline's streams on a hardware queue of its own: a stream with a CU mask gets one
// (all CUs here; tools/native/queue_map.cpp), where default streams share the process's 4 and two
// of the pipeline's could land on one, so a chunk's kernel queued behind the previous chunk's copy
// back. Such streams are blocking streams: they and the null stream wait on each other.
int Pipe::ensure(neb_engine* e) {
    if (!h2d || !comp || !d2h) {
        std::vector<uint32_t> mask(((uint32_t)e->cu_count + 31u) / 32u, 0u);
        for (int c = 0; c < e->cu_count; c++) mask[c / 32] |= 1u << (c % 32);
        for (neb::Stream* st : {&h2d, &comp, &d2h}) HIP_TRY(st->create_cu_mask((uint32_t)mask.size(), mask.data()));
    }
    // each create and reserve does nothing for what exists: a slot that a failure left half built is completed
    for (auto& s : slot) {
        for (neb::Event* ev : {&s.in_done, &s.k_done, &s.done}) HIP_TRY(ev->create(hipEventDisableTiming));
        HIP_TRY(s.h_desc.reserve(kPipeChunkPkts * sizeof(neb_desc)));
        HIP_TRY(s.d_desc.reserve(kPipeChunkPkts * sizeof(neb_desc)));
        HIP_TRY(s.h_status.reserve(kPipeChunkPkts * sizeof(int32_t)));
        s.count = 0;
    }
    return NEB_OK;
}

// The host waits for the chunk's copy back. In the trace each copy-in then starts as the copy back
// two chunks before it ends, 284 µs per call idle on the copy-in stream (profiles/r6/host/
// final_*_trace.csv, tools/r6/copy_overlap.py). Two ways of removing that wait measured no better
// and were removed: waiting for the copy back on the device, 27.9-29.3 against
// 31.7-33.4 GiB/s (ab_gpu_wait.jsonl); an empty kernel after each copy back with the event after
// it, 30.5-32.3 against 31.3-32.9 (ab_mark.jsonl).
hipError_t Pipe::retire(PipeSlot& s) {
    hipError_t err = hipEventSynchronize(s.done);
    if (err != hipSuccess) return err;
    std::memcpy(s.user_status + s.user_begin, s.h_status, s.count * sizeof(int32_t));
    s.count = 0;
    return hipSuccess;
}

void Pipe::drain() {
    for (const neb::Stream* st : {&h2d, &comp, &d2h})
        if (*st) (void)hipStreamSynchronize(*st);
    for (auto& s : slot) s.count = 0;
}

// Host-resident batch. A pinned, mapped arena runs zero-copy (above). Any other arena is staged in
// chunks of at most kPipeChunkPkts packets (pipe_plan) rotated over kPipeSlots device buffers: each
// chunk's arena span is copied in (hipMemcpyAsync), sealed/opened on the device and copied back on
// three streams, so one chunk's copy-in overlaps another's kernel and another's copy-back.
// NEB_HOST_MODE=dma forces the staging for a mapped arena too. Every descriptor is checked before
// anything is copied or launched: an invalid batch returns NEB_ERR_INVALID with the arena and the
// statuses untouched.
static int batch_host(neb_engine* e, int alg, int open, const neb_desc* desc, uint32_t n, uint8_t* arena,
                      size_t arena_len, int32_t* status, uint32_t key_hint) {
    int rc = check_batch(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (n == 0) return NEB_OK;
    if (!desc || !arena || !status) return NEB_ERR_INVALID;
    // Every descriptor is checked before the arena or the statuses are written. The staged path
    // checks the first chunk's, starts that chunk's copy-in and kernel (they write device buffers
    // only), and checks the rest while they run: ≈ 90 µs of checks per 64 Ki packets off the
    // critical path. Its first copy back waits for the whole check.
    uint32_t checked = 0;
    auto check_upto = [&](uint32_t end) {
        for (; checked < end; checked++)
            if (!neb_desc_in_arena(desc[checked], open, arena_len)) return false;
        return true;
    };
    std::lock_guard<std::mutex> g(e->pipe_mu);
    DeviceGuard dg(e->device);
    // The kernels' vector fast path tests the absolute address (arena base + offset), so a mapped
    // arena at any byte address runs zero-copy. A staged arena lands in a device buffer with the
    // same alignment modulo 16, so the kernels take the same paths either way.
    if (host_mode() == kHostZeroCopy && host_mapped(arena)) {
        if (!check_upto(n)) return NEB_ERR_INVALID;
        return batch_host_zero_copy(e, alg, open, desc, n, arena, arena_len, status, key_hint);
    }
    Pipe& P = e->pipe;
    if ((rc = P.ensure(e)) != NEB_OK) return rc;
    // any failure below leaves work queued on the three streams: drain them before returning
#define PIPE_TRY(x)                  \
    do {                             \
        hipError_t err_ = (x);       \
        if (err_ != hipSuccess) {    \
            set_error(#x, err_);     \
            P.drain();               \
            return NEB_ERR_HIP;      \
        }                            \
    } while (0)
    const std::vector<uint32_t> plan = neb::pipe_plan(n);
    uint32_t begin = 0;
    for (uint32_t k = 0; k < plan.size(); begin += plan[k], k++) {
        PipeSlot& s = P.slot[k % kPipeSlots];
        const uint32_t cnt = plan[k];
        if (s.count) PIPE_TRY(P.retire(s));  // the slot's previous chunk is back
        if (!check_upto(begin + cnt)) {      // (only ever the first chunk: the rest were checked after it)
            P.drain();
            return NEB_ERR_INVALID;
        }
        // A chunk copies its whole span back, so spans of chunks in flight must not overlap (the
        // descriptors need not be in arena order): retire any other slot whose span intersects.
        const neb::PipeSpan sp = neb::pipe_span(desc + begin, cnt, open);
        for (auto& o : P.slot)
            if (&o != &s && o.count && o.span.overlaps(sp)) PIPE_TRY(P.retire(o));
        const size_t bytes = (size_t)(sp.hi - sp.lo);
        PIPE_TRY(s.d_buf.reserve(align_up(bytes, 1 << 20)));  // (retired: nothing in flight uses it)
        neb::pipe_rebase(s.h_desc, desc + begin, cnt, sp.lo);
        s.span = sp;
        s.user_status = status;
        s.user_begin = begin;
        s.count = cnt;
        PIPE_TRY(hipMemcpyAsync(s.d_buf, arena + sp.lo, bytes, hipMemcpyHostToDevice, P.h2d));
        PIPE_TRY(hipEventRecord(s.in_done, P.h2d));
        // The kernels write the chunk's statuses in the slot's pinned, mapped buffer themselves (4 B
        // per packet of posted writes). Its descriptors go to the device on the kernels' stream,
        // ahead of them: read over PCIe in place they waited behind the copies' 90 GB/s, and the
        // kernels ran 250-478 µs per 16 Ki-packet chunk instead of ≈ 25 (profiles/r6/host/); on the
        // copy-in stream the small copy's latency left that stream idle between chunks.
        PIPE_TRY(hipStreamWaitEvent(P.comp, s.in_done, 0));
        PIPE_TRY(neb_copy_desc(s.d_desc, s.h_desc, cnt, P.comp));
        PIPE_TRY(launch_batch(e, {.alg = alg, .open = open, .desc = s.d_desc, .n = cnt, .arena = s.d_buf,
                                  .status = s.h_status, .key_hint = key_hint, .stream = P.comp, .sched = &P.sched}));
        PIPE_TRY(hipEventRecord(s.k_done, P.comp));
        if (k == 0 && !check_upto(n)) {  // the rest of the batch, while chunk 0 is copied in and run
            P.drain();
            return NEB_ERR_INVALID;
        }
        PIPE_TRY(hipStreamWaitEvent(P.d2h, s.k_done, 0));
        PIPE_TRY(hipMemcpyAsync(arena + sp.lo, s.d_buf, bytes, hipMemcpyDeviceToHost, P.d2h));
        PIPE_TRY(hipEventRecord(s.done, P.d2h));
    }
    for (auto& s : P.slot)
        if (s.count) PIPE_TRY(P.retire(s));
#undef PIPE_TRY
    return NEB_OK;
}

NEB_API int neb_seal_batch_host(neb_engine* e, int alg, const neb_desc* desc, uint32_t n, uint8_t* arena,
                                size_t arena_len, int32_t* status, uint32_t key_hint) {
    return batch_host(e, alg, 0, desc, n, arena, arena_len, status, key_hint);
}

NEB_API int neb_open_batch_host(neb_engine* e, int alg, const neb_desc* desc, uint32_t n, uint8_t* arena,
                                size_t arena_len, int32_t* status, uint32_t key_hint) {
    return batch_host(e, alg, 1, desc, n, arena, arena_len, status, key_hint);
}

// ---- the host receive's staging (window.cpp) --------------------------------------------------
// neb::RxStaging (engine_internal.hpp): active when the arena is mapped pinned memory and zero-copy
// is the host mode; e->rx is then the caller's until the object goes.

neb::RxStaging::RxStaging(neb_engine* e, int alg, uint32_t key_hint, uint8_t* arena, uint32_t n)
    : alg_(alg), rc_(check_batch(e, alg, key_hint)), key_hint_(key_hint), arena_(arena) {
    if (rc_ != NEB_OK || n == 0 || host_mode() != kHostZeroCopy || !host_mapped(arena)) return;
    auto& r = e->rx;
    std::unique_lock<std::mutex> lk(r.mu);
    hipSetDevice(e->device);
    rc_ = NEB_ERR_HIP;
    // the kernels' stores into the mapped arena must be visible to the host at the event
    if (r.stream.create(hipStreamNonBlocking) != hipSuccess ||
        r.ev.create(hipEventDisableTiming | hipEventReleaseToSystem) != hipSuccess)
        return;
    // a staging buffer is freed (to grow) only with the receive stream idle: nothing queued reads it
    auto idle = [&] { return hipStreamSynchronize(r.stream); };
    if (r.h_desc.reserve((size_t)n * sizeof(neb_desc), nullptr, idle) != hipSuccess ||
        r.h_status.reserve((size_t)n * sizeof(int32_t), nullptr, idle) != hipSuccess ||
        r.d_desc.reserve((size_t)n * sizeof(neb_desc), nullptr, idle) != hipSuccess ||
        r.d_status.reserve((size_t)n * sizeof(int32_t), nullptr, idle) != hipSuccess)
        return;
    rc_ = NEB_OK;
    desc_ = r.h_desc;
    status_ = r.h_status;
    e_ = e;
    lk.release();  // held until ~RxStaging
}

int neb::RxStaging::open(uint32_t cnt) {
    auto& r = e_->rx;
    HIP_TRY(hipMemcpyAsync(r.d_desc, r.h_desc, (size_t)cnt * sizeof(neb_desc), hipMemcpyHostToDevice, r.stream));
    HIP_TRY(launch_batch(e_, {.alg = alg_, .open = 1, .desc = r.d_desc, .n = cnt, .arena = arena_, .status = r.d_status,
                              .key_hint = key_hint_, .stream = r.stream, .sched = &r.sched}));
    HIP_TRY(hipMemcpyAsync(r.h_status, r.d_status, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    HIP_TRY(hipEventRecord(r.ev, r.stream));
    HIP_TRY(hipEventSynchronize(r.ev));
    return NEB_OK;
}

neb::RxStaging::~RxStaging() {
    if (!e_) return;
    hipStreamSynchronize(e_->rx.stream);
    e_->rx.mu.unlock();
}

// ---- transmit batch (tx.hip) ------------------------------------------------------------------

static hipError_t tx_reserve(neb_engine* e, uint32_t n, uint32_t ntun, uint32_t max_wires) {
    TxSpace& tx = e->tx;
    if (tx.dev.mem() && n <= tx.n_cap && ntun <= tx.tun_cap && max_wires <= tx.wire_cap) return hipSuccess;
    const uint32_t nc = std::max({n, tx.n_cap, 1024u}), tc = std::max({ntun, tx.tun_cap, 64u});
    const uint32_t wc = std::max({max_wires, tx.wire_cap, 1024u});
    size_t cub = 0;
    const size_t bytes = neb_tx_ws_bytes(nc, tc, wc, &cub);
    tx.n_cap = tx.tun_cap = tx.wire_cap = 0;
    hipError_t err = tx.dev.reserve(bytes);  // (laid out again whether it grew or not: the capacities changed)
    if (err != hipSuccess) return err;
    neb::tx_ws_layout(nc, tc, wc, cub, tx.dev.mem(), &tx.ws);
    tx.n_cap = nc;
    tx.tun_cap = tc;
    tx.wire_cap = wc;
    return hipSuccess;
}

// caller holds e->tx.mu
// d_via (optional): the tunnels' relays (neb_tx_seal_via_batch)
static int tx_run(neb_engine* e, int alg, neb_tx_tunnel* d_tun, uint32_t ntun, const neb_relay_route* d_via,
                  const neb_tx_packet* d_pk, uint32_t npk, const uint8_t* d_in, uint8_t* d_out, size_t out_cap,
                  neb_tx_wire* d_wires, int32_t* d_wire_status, uint32_t max_wires, uint32_t* d_nwires,
                  int32_t* d_pk_status, uint32_t key_hint, hipStream_t s) {
    TxSpace& tx = e->tx;
    HIP_TRY(tx_reserve(e, npk, ntun, max_wires));
    HIP_TRY(tx.dev.begin(s));
    if (d_via) {
        // the relay tunnels' one key, for a single-key outer seal: asked for first, read back after
        // the inner seal is enqueued, so the host waits for this word only while the device works
        HIP_TRY(tx.h_via_key.reserve(sizeof(uint32_t)));
        HIP_TRY(tx.via_ev.create(hipEventDisableTiming));
        HIP_TRY(neb_tx_via_key(d_tun, ntun, d_via, tx.h_via_key, s));
        HIP_TRY(hipEventRecord(tx.via_ev, s));
    }
    HIP_TRY(neb_tx_plan(d_pk, npk, d_in, d_tun, ntun, d_via, e->d_keys, e->max_keys, alg, &tx.ws, out_cap, max_wires,
                        d_pk_status, d_nwires, s));
    // one tunnel key with AES-GCM: the seal sums the payload into the L4 checksums itself, so the
    // segment kernel does not read the payload (gcm_packet.hpp gcm_csum_fix)
    const bool cs = alg == NEB_ALG_AESGCM && key_hint != NEB_KEYS_MIXED;
    const uint32_t cs_slots = cs ? neb_gcm_single_slots(max_wires, e->cu_count, 0, 2) : 0u;
    HIP_TRY(neb_tx_segment(d_pk, npk, d_in, d_tun, d_via, d_out, &tx.ws, d_wires, d_nwires, max_wires, e->cu_count,
                           cs_slots, s));
    HIP_TRY(launch_batch(e, {.alg = alg, .open = 0, .desc = tx.ws.seal_desc, .n = max_wires, .d_n = d_nwires,
                             .arena = d_out, .status = d_wire_status, .key_hint = key_hint, .stream = s,
                             .hdr_from_dst = cs ? 2 : 1}));  // the seal reads the payload from the TUN read
    HIP_TRY(neb_tx_finish(d_tun, npk, ntun, &tx.ws, s));
    if (d_via && max_wires) {
        // prepareSendVia's tags: the AD-only seal over the compacted via wires, behind the inner seal
        HIP_TRY(hipEventSynchronize(tx.via_ev));
        uint32_t hint = *tx.h_via_key;
        if (hint != NEB_KEYS_MIXED && check_batch(e, alg, hint) != NEB_OK) hint = NEB_KEYS_MIXED;
        HIP_TRY(launch_batch(e, {.alg = alg, .open = 0, .desc = tx.ws.via_desc, .n = max_wires, .d_n = tx.ws.nvia,
                                 .arena = d_out, .status = tx.ws.via_status, .key_hint = hint, .stream = s}));
        HIP_TRY(neb_tx_via_fix(&tx.ws, max_wires, d_wire_status, s));
        note_use(e, hint, s);
    }
    HIP_TRY(tx.dev.end(s));
    return NEB_OK;
}

static int tx_device(neb_engine* e, int alg, neb_tx_tunnel* d_tunnels, uint32_t ntunnels, const neb_relay_route* d_via,
                     const neb_tx_packet* d_packets, uint32_t npackets, const uint8_t* d_in, uint8_t* d_out,
                     size_t out_cap, neb_tx_wire* d_wires, int32_t* d_wire_status, uint32_t max_wires,
                     uint32_t* d_nwires, int32_t* d_packet_status, uint32_t key_hint, void* stream) {
    int rc = check_batch(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (!d_nwires || (npackets && (!d_packets || !d_in || !d_packet_status || !d_tunnels)) ||
        (max_wires && (!d_out || !d_wires || !d_wire_status)))
        return NEB_ERR_INVALID;
    DeviceGuard dg(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (npackets == 0) {
        HIP_TRY(hipMemsetAsync(d_nwires, 0, sizeof(uint32_t), s));
        return NEB_OK;
    }
    std::lock_guard<std::mutex> g(e->tx.mu);
    rc = tx_run(e, alg, d_tunnels, ntunnels, d_via, d_packets, npackets, d_in, d_out, out_cap, d_wires, d_wire_status,
                max_wires, d_nwires, d_packet_status, key_hint, s);
    if (rc == NEB_OK) note_use(e, key_hint, s);
    return rc;
}

NEB_API int neb_tx_seal_batch(neb_engine* e, int alg, neb_tx_tunnel* d_tunnels, uint32_t ntunnels,
                              const neb_tx_packet* d_packets, uint32_t npackets, const uint8_t* d_in,
                              uint8_t* d_out, size_t out_cap, neb_tx_wire* d_wires, int32_t* d_wire_status,
                              uint32_t max_wires, uint32_t* d_nwires, int32_t* d_packet_status, uint32_t key_hint,
                              void* stream) {
    return tx_device(e, alg, d_tunnels, ntunnels, nullptr, d_packets, npackets, d_in, d_out, out_cap, d_wires,
                     d_wire_status, max_wires, d_nwires, d_packet_status, key_hint, stream);
}

NEB_API int neb_tx_seal_via_batch(neb_engine* e, int alg, neb_tx_tunnel* d_tunnels, uint32_t ntunnels,
                                  const neb_relay_route* d_via, const neb_tx_packet* d_packets, uint32_t npackets,
                                  const uint8_t* d_in, uint8_t* d_out, size_t out_cap, neb_tx_wire* d_wires,
                                  int32_t* d_wire_status, uint32_t max_wires, uint32_t* d_nwires,
                                  int32_t* d_packet_status, uint32_t key_hint, void* stream) {
    return tx_device(e, alg, d_tunnels, ntunnels, ntunnels ? d_via : nullptr, d_packets, npackets, d_in, d_out, out_cap,
                     d_wires, d_wire_status, max_wires, d_nwires, d_packet_status, key_hint, stream);
}

static int tx_host(neb_engine* e, int alg, neb_tx_tunnel* tunnels, uint32_t ntunnels, const neb_relay_route* via,
                   const neb_tx_packet* packets, uint32_t npackets, const uint8_t* in, size_t in_len, uint8_t* out,
                   size_t out_cap, neb_tx_wire* wires, int32_t* wire_status, uint32_t max_wires, uint32_t* nwires,
                   int32_t* packet_status, uint32_t key_hint) {
    int rc = check_batch(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (!nwires || (npackets && (!packets || !in || !packet_status || (ntunnels && !tunnels))) ||
        (max_wires && (!out || !wires || !wire_status)))
        return NEB_ERR_INVALID;
    *nwires = 0;
    if (npackets == 0) return NEB_OK;
    // the input span the packets touch, uploaded once
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < npackets; i++) {
        if (!span_in(packets[i].in_off, packets[i].len, in_len)) return NEB_ERR_INVALID;
        lo = std::min(lo, packets[i].in_off);
        hi = std::max(hi, packets[i].in_off + packets[i].len);
    }
    lo &= ~(uint64_t)15;
    const size_t span = (size_t)(hi - lo);
    const size_t o_tun = 0, o_pk = align_up((size_t)ntunnels * sizeof(neb_tx_tunnel), 256);
    const size_t o_in = o_pk + align_up((size_t)npackets * sizeof(neb_tx_packet), 256);
    const size_t o_out = o_in + align_up(span, 256);
    const size_t o_w = o_out + align_up(out_cap, 256);
    const size_t o_ws = o_w + align_up((size_t)max_wires * sizeof(neb_tx_wire), 256);
    const size_t o_ps = o_ws + align_up((size_t)max_wires * 4, 256);
    const size_t o_n = o_ps + align_up((size_t)npackets * 4, 256);
    const size_t o_via = o_n + 256;
    const size_t total = o_via + (via ? align_up((size_t)ntunnels * sizeof(neb_relay_route), 256) : 0);
    std::vector<neb_tx_packet> rebased(packets, packets + npackets);
    for (auto& p : rebased) p.in_off -= lo;
    std::lock_guard<std::mutex> g(e->tx.mu);
    DeviceGuard dg(e->device);
    TxSpace& tx = e->tx;
    hipStream_t s = e->stream;
    HIP_TRY(tx.dev.reserve(align_up(total, 1 << 20), nullptr, TxSpace::kIo));
    uint8_t* d = tx.dev.mem(TxSpace::kIo);
    auto* d_tun = (neb_tx_tunnel*)(d + o_tun);
    auto* d_pk = (neb_tx_packet*)(d + o_pk);
    auto* d_wires = (neb_tx_wire*)(d + o_w);
    auto* d_wst = (int32_t*)(d + o_ws);
    auto* d_pst = (int32_t*)(d + o_ps);
    auto* d_n = (uint32_t*)(d + o_n);
    if (ntunnels) HIP_TRY(hipMemcpyAsync(d_tun, tunnels, ntunnels * sizeof(neb_tx_tunnel), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_pk, rebased.data(), npackets * sizeof(neb_tx_packet), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + o_in, in + lo, span, hipMemcpyHostToDevice, s));
    auto* d_via = via ? (neb_relay_route*)(d + o_via) : nullptr;
    if (via) HIP_TRY(hipMemcpyAsync(d_via, via, ntunnels * sizeof(neb_relay_route), hipMemcpyHostToDevice, s));
    rc = tx_run(e, alg, d_tun, ntunnels, d_via, d_pk, npackets, d + o_in, d + o_out, out_cap, d_wires, d_wst, max_wires,
                d_n, d_pst, key_hint, s);
    if (rc != NEB_OK) return rc;
    unsigned long long tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tot, tx.ws.totals, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(packet_status, d_pst, npackets * 4, hipMemcpyDeviceToHost, s));
    if (ntunnels) HIP_TRY(hipMemcpyAsync(tunnels, d_tun, ntunnels * sizeof(neb_tx_tunnel), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t nw = (uint32_t)tot[0];
    if (nw) {
        HIP_TRY(hipMemcpyAsync(wires, d_wires, nw * sizeof(neb_tx_wire), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(wire_status, d_wst, nw * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out, d + o_out, (size_t)tot[1], hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *nwires = nw;
    return NEB_OK;
}

NEB_API int neb_tx_seal_batch_host(neb_engine* e, int alg, neb_tx_tunnel* tunnels, uint32_t ntunnels,
                                   const neb_tx_packet* packets, uint32_t npackets, const uint8_t* in, size_t in_len,
                                   uint8_t* out, size_t out_cap, neb_tx_wire* wires, int32_t* wire_status,
                                   uint32_t max_wires, uint32_t* nwires, int32_t* packet_status, uint32_t key_hint) {
    return tx_host(e, alg, tunnels, ntunnels, nullptr, packets, npackets, in, in_len, out, out_cap, wires, wire_status,
                   max_wires, nwires, packet_status, key_hint);
}

NEB_API int neb_tx_seal_via_batch_host(neb_engine* e, int alg, neb_tx_tunnel* tunnels, uint32_t ntunnels,
                                       const neb_relay_route* via, const neb_tx_packet* packets, uint32_t npackets,
                                       const uint8_t* in, size_t in_len, uint8_t* out, size_t out_cap,
                                       neb_tx_wire* wires, int32_t* wire_status, uint32_t max_wires,
                                       uint32_t* nwires, int32_t* packet_status, uint32_t key_hint) {
    return tx_host(e, alg, tunnels, ntunnels, ntunnels ? via : nullptr, packets, npackets, in, in_len, out, out_cap,
                   wires, wire_status, max_wires, nwires, packet_status, key_hint);
}

// ---- receive coalescer (coalesce.hip) -----------------------------------------------------------

static hipError_t co_reserve(neb_engine* e, uint32_t n) {
    CoSpace& co = e->co;
    if (co.dev.mem() && n <= co.n_cap) return hipSuccess;
    const uint32_t nc = std::max({n, co.n_cap, 1024u});
    size_t cub = 0;
    const size_t bytes = neb_co_ws_bytes(nc, &cub);
    co.n_cap = 0;
    hipError_t err = co.dev.reserve(bytes);  // (laid out again whether it grew or not: the capacity changed)
    if (err != hipSuccess) return err;
    neb::co_ws_layout(nc, cub, co.dev.mem(), &co.ws);
    co.n_cap = nc;
    return hipSuccess;
}

NEB_API int neb_rx_coalesce_batch(neb_engine* e, const neb_plain_packet* d_plain, uint32_t n, const uint8_t* d_in,
                                  uint8_t* d_out, size_t out_cap, neb_tun_write* d_writes, uint32_t max_writes,
                                  uint32_t* d_nwrites, uint32_t* d_pkt_write, int32_t* d_pkt_status, uint32_t lanes,
                                  void* stream) {
    if (!e || !d_nwrites || (n && (!d_plain || !d_in || !d_pkt_write || !d_pkt_status)) ||
        (max_writes && !d_writes) || (out_cap && !d_out) || n > 0x7FFFFFFFu ||
        (lanes & ~(uint32_t)(NEB_COALESCE_TCP | NEB_COALESCE_UDP)))
        return NEB_ERR_INVALID;
    DeviceGuard dg(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_nwrites, 0, sizeof(uint32_t), s));
        return NEB_OK;
    }
    const int64_t hb = neb::knob(NEB_KNOB_COALESCE_HASH_BITS);
    std::lock_guard<std::mutex> g(e->co.mu);
    CoSpace& co = e->co;
    HIP_TRY(co_reserve(e, n));
    HIP_TRY(co.dev.begin(s));
    HIP_TRY(neb_co_run(d_plain, n, d_in, d_out, out_cap, d_writes, max_writes, d_nwrites, d_pkt_write, d_pkt_status,
                       lanes, hb < 0 ? 0u : hb > 32 ? 32u : (uint32_t)hb, &co.ws, s));
    HIP_TRY(co.dev.end(s));
    return NEB_OK;
}

NEB_API int neb_rx_plain_from_wire(neb_engine* e, const neb_rx_packet* d_pk, const int32_t* d_status,
                                   const uint64_t* d_epoch, uint32_t nepoch, uint32_t n, const uint8_t* d_arena,
                                   neb_plain_packet* d_plain, void* stream) {
    if (!e || (n && (!d_pk || !d_status || !d_arena || !d_plain)) || (nepoch && !d_epoch)) return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    DeviceGuard dg(e->device);
    HIP_TRY(neb_co_plain_from_wire(d_pk, d_status, d_epoch, nepoch, n, d_arena, d_plain, (hipStream_t)stream));
    return NEB_OK;
}

// ---- TX send plan (send.hip) ---------------------------------------------------------------------

static hipError_t send_reserve(neb_engine* e, uint32_t n) {
    SendSpace& sp = e->send;
    if (sp.dev.mem() && n <= sp.n_cap) return hipSuccess;
    const uint32_t nc = std::max({n, sp.n_cap, 1024u});
    size_t cub = 0;
    const size_t bytes = neb_send_ws_bytes(nc, &cub);
    sp.n_cap = 0;
    hipError_t err = sp.dev.reserve(bytes);  // (laid out again whether it grew or not: the capacity changed)
    if (err != hipSuccess) return err;
    neb::send_ws_layout(nc, cub, sp.dev.mem(), &sp.ws);
    sp.n_cap = nc;
    return hipSuccess;
}

NEB_API int neb_tx_send_plan(neb_engine* e, const neb_tx_wire* d_wires, const int32_t* d_wire_status,
                             const uint32_t* d_nwires, uint32_t max_wires, const neb_tx_packet* d_packets,
                             uint32_t npackets, const neb_relay_route* d_via, const neb_udp_addr* d_remote,
                             uint32_t ntunnels, uint32_t socket_v4, uint32_t max_segments, uint32_t chunk_packets,
                             neb_send_iov* d_iov, uint32_t* d_niov, neb_send_entry* d_entries, uint32_t* d_nentries,
                             uint32_t* d_wire_entry, int32_t* d_send_status, void* stream) {
    if (!e || max_segments > neb::kSendMaxSegments || max_wires > 0x7FFFFFFFu || !d_nwires || !d_niov || !d_nentries ||
        (npackets && !d_packets) || (ntunnels && !d_remote) || (reinterpret_cast<uintptr_t>(d_remote) & 3u) ||
        (reinterpret_cast<uintptr_t>(d_iov) & 7u) ||
        (max_wires && (!d_wires || !d_wire_status || !d_iov || !d_entries || !d_wire_entry || !d_send_status)))
        return NEB_ERR_INVALID;
    if (max_wires == 0) return NEB_OK;
    DeviceGuard dg(e->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(e->send.mu);
    SendSpace& sp = e->send;
    HIP_TRY(send_reserve(e, max_wires));
    HIP_TRY(sp.dev.begin(s));
    neb::SendArgs a{d_wires, d_wire_status, d_nwires, d_packets, d_via, d_remote, d_iov, d_niov, d_entries, d_nentries,
                    d_wire_entry, d_send_status, max_wires, npackets, ntunnels, socket_v4, max_segments, chunk_packets,
                    sp.ws};
    HIP_TRY(neb_send_run(&a, s));
    HIP_TRY(sp.dev.end(s));
    return NEB_OK;
}

// ---- RX receive plan (recv.hip) ------------------------------------------------------------------

static hipError_t recv_reserve(neb_engine* e, uint32_t n) {
    RecvSpace& sp = e->recv;
    if (sp.dev.mem() && n <= sp.n_cap) return hipSuccess;
    const uint32_t nc = std::max({n, sp.n_cap, 1024u});
    size_t cub = 0;
    const size_t bytes = neb_recv_ws_bytes(nc, &cub);
    sp.n_cap = 0;
    hipError_t err = sp.dev.reserve(bytes);  // (laid out again whether it grew or not: the capacity changed)
    if (err != hipSuccess) return err;
    neb::recv_ws_layout(nc, cub, sp.dev.mem(), &sp.ws);
    sp.n_cap = nc;
    return hipSuccess;
}

NEB_API int neb_rx_recv_plan(neb_engine* e, const neb_recv_entry* d_entries, uint32_t nentries, const uint8_t* d_ctrl,
                             uint32_t ctrl_stride, uint32_t socket_v4, neb_rx_packet* d_pk, neb_rx_source* d_src,
                             uint32_t* d_pkt_entry, uint32_t max_packets, neb_udp_addr* d_from, uint32_t* d_entry_first,
                             uint32_t* d_counts, void* stream) {
    if (!e || !d_pk || !d_entry_first || !d_counts || (nentries && !d_entries) || nentries > 0x7FFFFFFFu ||
        max_packets > 0x7FFFFFFFu ||
        (d_ctrl && (ctrl_stride == 0u || (ctrl_stride & 7u) || ctrl_stride > neb::kRecvMaxCtrlStride)) ||
        (reinterpret_cast<uintptr_t>(d_entries) & 7u) || (reinterpret_cast<uintptr_t>(d_ctrl) & 7u))
        return NEB_ERR_INVALID;
    DeviceGuard dg(e->device);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(e->recv.mu);
    RecvSpace& sp = e->recv;
    HIP_TRY(recv_reserve(e, nentries));
    HIP_TRY(sp.dev.begin(s));
    neb::RecvArgs a{d_entries, d_ctrl, d_pk, d_src, d_pkt_entry, d_from, d_entry_first, d_counts,
                    nentries, max_packets, ctrl_stride, socket_v4, sp.ws};
    HIP_TRY(neb_recv_run(&a, s));
    HIP_TRY(sp.dev.end(s));
    return NEB_OK;
}

// ---- RX batch report (report.hip) ------------------------------------------------------------------

static hipError_t report_reserve(neb_engine* e, uint32_t n) {
    ReportSpace& sp = e->report;
    if (sp.dev.mem() && n <= sp.n_cap) return hipSuccess;
    const uint32_t nc = std::max({n, sp.n_cap, 1024u});
    size_t cub = 0;
    const size_t bytes = neb_report_ws_bytes(nc, &cub);
    sp.n_cap = 0;
    hipError_t err = sp.dev.reserve(bytes);  // (laid out again whether it grew or not: the capacity changed)
    if (err != hipSuccess) return err;
    neb::report_ws_layout(nc, cub, sp.dev.mem(), &sp.ws);
    sp.n_cap = nc;
    return hipSuccess;
}

NEB_API int neb_rx_report_batch(neb_engine* e, const neb_rx_packet* d_pk, const int32_t* d_status, uint32_t n,
                                const uint8_t* d_arena, const neb_udp_addr* d_from, const uint32_t* d_pkt_entry, uint32_t nfrom,
                                uint32_t flags, neb_rx_run* d_runs, neb_rx_relay_used* d_relay_used, neb_rx_work* d_work,
                                uint64_t* d_metrics, uint32_t* d_counts, void* stream) {
    auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if (!e || !d_metrics || !d_counts || n > 0x7FFFFFFFu || (flags & ~NEB_REPORT_RELAYED) ||
        (n && (!d_pk || !d_status || !d_arena || !d_runs || !d_relay_used || !d_work)) ||
        ((at(d_runs) | at(d_metrics)) & 7u) ||
        ((at(d_pk) | at(d_status) | at(d_from) | at(d_pkt_entry) | at(d_relay_used) | at(d_work) | at(d_counts)) & 3u))
        return NEB_ERR_INVALID;
    DeviceGuard dg(e->device);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_metrics, 0, neb::kReportMetrics * sizeof(uint64_t), s));
        HIP_TRY(hipMemsetAsync(d_counts, 0, 4 * sizeof(uint32_t), s));
        return NEB_OK;
    }
    std::lock_guard<std::mutex> g(e->report.mu);
    ReportSpace& sp = e->report;
    HIP_TRY(report_reserve(e, n));
    HIP_TRY(sp.dev.begin(s));
    neb::ReportArgs a{d_pk, d_status, d_arena, d_from, d_pkt_entry, d_runs, d_relay_used, d_work, d_metrics, d_counts,
                      n, nfrom, flags & NEB_REPORT_RELAYED, sp.ws};
    HIP_TRY(neb_report_run(&a, s));
    HIP_TRY(sp.dev.end(s));
    return NEB_OK;
}

// ---- several engines --------------------------------------------------------------

// One tunnel key is one install on every engine (a tunnel has exactly one eKey / dKey,
// connection_state.go:37-49): shard k may use a key slot only if engine k holds there the same
// install (slot_tag) as engine 0, whose key table defines the batch's keys. Keys put on every
// engine by one neb_cipher_create_multi agree; anything else — a slot destroyed and reinstalled
// on one engine, keys installed engine by engine — does not, and the packets of shard k that name
// such a slot get NEB_STATUS_BAD_KEY instead of being sealed or opened with another tunnel's key.
// bad[k] flags engine k's disagreeing slots (empty when all agree; any = some engine disagrees).
struct KeyFence {
    std::vector<std::vector<uint8_t>> bad;
    bool any = false;
    bool bad_key(uint32_t k, uint32_t key) const { return key < bad[k].size() && bad[k][key]; }
};
static KeyFence key_fence(neb_engine* const* es, uint32_t m) {
    KeyFence f;
    f.bad.resize(m);
    std::vector<neb_engine*> order(es, es + m);
    std::sort(order.begin(), order.end());
    order.erase(std::unique(order.begin(), order.end()), order.end());
    if (order.size() < 2) return f;
    for (neb_engine* e : order) e->key_mu.lock();
    for (uint32_t k = 1; k < m; k++) {
        neb_engine* a = es[0];
        neb_engine* b = es[k];
        if (a == b) continue;
        const uint32_t nk = std::max(a->max_keys, b->max_keys);
        std::vector<uint8_t> v(nk, 0);
        bool anyk = false;
        for (uint32_t s = 0; s < nk; s++) {
            const uint64_t ta = s < a->max_keys ? a->slot_tag[s] : 0, tb = s < b->max_keys ? b->slot_tag[s] : 0;
            const int aa = s < a->max_keys ? a->slot_alg[s] : 0, ab = s < b->max_keys ? b->slot_alg[s] : 0;
            if (ta != tb || aa != ab) v[s] = 1, anyk = true;
        }
        if (anyk) {
            f.bad[k] = std::move(v);
            f.any = true;
        }
    }
    for (neb_engine* e : order) e->key_mu.unlock();
    if (f.any) {  // the call still returns NEB_OK (the packets carry NEB_STATUS_BAD_KEY): say why
        uint32_t first = 0, slots = 0;
        for (uint32_t k = m; k-- > 1;)
            if (!f.bad[k].empty()) first = k;
        for (uint8_t x : f.bad[first]) slots += x;
        std::snprintf(g_last_error, sizeof g_last_error,
                      "key fence: engine %u holds other installs than engine 0 in %u key slot(s); their packets get "
                      "NEB_STATUS_BAD_KEY (install a tunnel key on every engine with neb_cipher_create_multi)",
                      first, slots);
    }
    return f;
}

// Shard k of m: packets [n*k/m, n*(k+1)/m).
static inline uint32_t shard_lo(uint32_t n, uint32_t k, uint32_t m) { return (uint32_t)((uint64_t)n * k / m); }

static int batch_host_multi(neb_engine* const* engines, uint32_t m, int alg, int open, const neb_desc* desc,
                            uint32_t n, uint8_t* arena, size_t arena_len, int32_t* status, uint32_t key_hint) {
    if (!engines || m == 0 || (n && (!desc || !arena || !status))) return NEB_ERR_INVALID;
    for (uint32_t k = 0; k < m; k++)
        if (!engines[k]) return NEB_ERR_INVALID;
    // every descriptor checked before any shard starts: an invalid batch touches nothing
    for (uint32_t i = 0; i < n; i++)
        if (!neb_desc_in_arena(desc[i], open, arena_len)) return NEB_ERR_INVALID;
    DeviceGuard dg;
    const KeyFence fence = key_fence(engines, m);
    // a shard whose engine disagrees on some keys runs on a copy of its descriptors with those
    // packets' key_id pointing past every key table (the kernels give them NEB_STATUS_BAD_KEY); a
    // single-key shard whose key disagrees is refused whole without a launch
    std::vector<std::vector<neb_desc>> fenced(m);
    std::vector<uint8_t> skip(m, 0);
    if (fence.any)
        for (uint32_t k = 1; k < m; k++) {
            if (fence.bad[k].empty()) continue;
            const uint32_t b = shard_lo(n, k, m), c = shard_lo(n, k + 1, m) - b;
            if (key_hint != NEB_KEYS_MIXED) {
                if (fence.bad_key(k, key_hint)) {
                    skip[k] = 1;
                    for (uint32_t i = 0; i < c; i++) status[b + i] = NEB_STATUS_BAD_KEY;
                }
                continue;
            }
            fenced[k].assign(desc + b, desc + b + c);
            for (neb_desc& d : fenced[k])
                if (fence.bad_key(k, d.key_id)) d.key_id = NEB_KEYS_MIXED - 1u;
        }
    auto run = [&](uint32_t k) -> int {
        const uint32_t b = shard_lo(n, k, m), c = shard_lo(n, k + 1, m) - b;
        if (skip[k]) return NEB_OK;
        const neb_desc* dk = fenced[k].empty() ? desc + b : fenced[k].data();
        return batch_host(engines[k], alg, open, dk, c, arena, arena_len, status + b, key_hint);
    };
    // A staged (not zero-copy) shard copies its whole arena span [lo & ~15, hi) in and back. Shards
    // whose spans meet (packed, unaligned or interleaved descriptors) would write stale bytes over
    // each other's results, so they run one after another; disjoint spans run side by side.
    bool serial = false;
    if (!(host_mode() == kHostZeroCopy && host_mapped(arena))) {
        std::vector<std::pair<uint64_t, uint64_t>> span;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t b = shard_lo(n, k, m), c = shard_lo(n, k + 1, m) - b;
            if (c == 0 || skip[k]) continue;
            const neb::PipeSpan sp = neb::pipe_span(desc + b, c, open);
            span.push_back({sp.lo, sp.hi});
        }
        std::sort(span.begin(), span.end());
        for (size_t i = 1; i < span.size(); i++)
            if (span[i].first < span[i - 1].second) serial = true;
    }
    std::vector<int> rc(m, NEB_OK);
    if (serial) {
        for (uint32_t k = 0; k < m; k++) rc[k] = run(k);
    } else {
        std::vector<std::thread> th;
        for (uint32_t k = 1; k < m; k++) th.emplace_back([&, k] { rc[k] = run(k); });
        rc[0] = run(0);
        for (auto& t : th) t.join();
    }
    for (int r : rc)
        if (r != NEB_OK) return r;
    return NEB_OK;
}

NEB_API int neb_seal_batch_host_multi(neb_engine* const* engines, uint32_t nengines, int alg, const neb_desc* desc,
                                      uint32_t n, uint8_t* arena, size_t arena_len, int32_t* status,
                                      uint32_t key_hint) {
    return batch_host_multi(engines, nengines, alg, 0, desc, n, arena, arena_len, status, key_hint);
}

NEB_API int neb_open_batch_host_multi(neb_engine* const* engines, uint32_t nengines, int alg, const neb_desc* desc,
                                      uint32_t n, uint8_t* arena, size_t arena_len, int32_t* status,
                                      uint32_t key_hint) {
    return batch_host_multi(engines, nengines, alg, 1, desc, n, arena, arena_len, status, key_hint);
}

static int batch_sharded(int alg, int open, const neb_shard* sh, uint32_t m, uint32_t key_hint) {
    if (!sh || m == 0) return NEB_ERR_INVALID;
    for (uint32_t k = 0; k < m; k++)
        if (!sh[k].e) return NEB_ERR_INVALID;
    DeviceGuard dg;
    std::vector<neb_engine*> es(m);
    for (uint32_t k = 0; k < m; k++) es[k] = sh[k].e;
    const KeyFence fence = key_fence(es.data(), m);
    // device copies of a fenced shard's descriptors (KeyFence; batch_host_multi), freed on return
    std::vector<DevBuf<>> temps;
    int rc = NEB_OK;
    uint32_t launched = 0;
    for (; launched < m && rc == NEB_OK; launched++) {  // every shard queued first, then all waited for
        const neb_shard& s = sh[launched];
        const neb_desc* d_desc = s.d_desc;
        if (fence.any && !fence.bad[launched].empty() && s.n) {
            hipSetDevice(s.e->device);
            hipStream_t st = (hipStream_t)s.stream;
            if (key_hint != NEB_KEYS_MIXED) {
                if (fence.bad_key(launched, key_hint)) {
                    if (!s.d_status || hipMemsetD32Async((hipDeviceptr_t)s.d_status, NEB_STATUS_BAD_KEY, s.n, st) !=
                                           hipSuccess)
                        rc = s.d_status ? NEB_ERR_HIP : NEB_ERR_INVALID;
                    continue;
                }
            } else {
                const std::vector<uint8_t>& bad = fence.bad[launched];
                const size_t db = align_up((size_t)s.n * sizeof(neb_desc), 256);
                if (!s.d_desc || temps.emplace_back().reserve(db + bad.size()) != hipSuccess) {
                    rc = s.d_desc ? NEB_ERR_HIP : NEB_ERR_INVALID;
                    continue;
                }
                uint8_t* t = temps.back();
                uint8_t* d_bad = t + db;
                if (hipMemcpyAsync(d_bad, bad.data(), bad.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
                    neb_fence_keys(s.d_desc, (neb_desc*)t, s.n, d_bad, (uint32_t)bad.size(), st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess) {  // `bad` is pageable and local
                    rc = NEB_ERR_HIP;
                    continue;
                }
                d_desc = (const neb_desc*)t;
            }
        }
        rc = batch_device(s.e, alg, open, d_desc, s.n, s.d_arena, s.d_status, key_hint, s.stream);
    }
    for (uint32_t k = 0; k < launched; k++) {
        hipSetDevice(sh[k].e->device);
        const hipError_t err = hipStreamSynchronize((hipStream_t)sh[k].stream);
        if (err != hipSuccess && rc == NEB_OK) {
            set_error("sharded batch", err);
            rc = NEB_ERR_HIP;
        }
    }
    return rc;
}

NEB_API int neb_seal_batch_sharded(int alg, const neb_shard* shards, uint32_t nshards, uint32_t key_hint) {
    return batch_sharded(alg, 0, shards, nshards, key_hint);
}

NEB_API int neb_open_batch_sharded(int alg, const neb_shard* shards, uint32_t nshards, uint32_t key_hint) {
    return batch_sharded(alg, 1, shards, nshards, key_hint);
}

NEB_API int neb_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return NEB_ERR_INVALID;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? NEB_OK : NEB_ERR_HIP;
}

NEB_API int neb_host_free(void* p) {
    if (!p) return NEB_ERR_INVALID;
    return hipHostFree(p) == hipSuccess ? NEB_OK : NEB_ERR_HIP;
}

// header/header.go:102-110
NEB_API void neb_header_encode(uint8_t b[16], uint8_t version, uint8_t type, uint8_t subtype, uint32_t remote_index,
                               uint64_t counter) {
    b[0] = (uint8_t)(version << 4 | (type & 0x0f));
    b[1] = subtype;
    b[2] = 0;
    b[3] = 0;
    for (int i = 0; i < 4; i++) b[4 + i] = (uint8_t)(remote_index >> (24 - 8 * i));
    for (int i = 0; i < 8; i++) b[8 + i] = (uint8_t)(counter >> (56 - 8 * i));
}

// header/header.go:143-156
NEB_API int neb_header_parse(const uint8_t* b, size_t len, uint8_t* version, uint8_t* type, uint8_t* subtype,
                             uint16_t* reserved, uint32_t* remote_index, uint64_t* counter) {
    if (!b || len < NEB_HEADER_LEN) return NEB_ERR_INVALID;
    if (version) *version = (b[0] >> 4) & 0x0f;
    if (type) *type = b[0] & 0x0f;
    if (subtype) *subtype = b[1];
    if (reserved) *reserved = (uint16_t)(b[2] << 8 | b[3]);
    if (remote_index) *remote_index = (uint32_t)b[4] << 24 | (uint32_t)b[5] << 16 | (uint32_t)b[6] << 8 | b[7];
    if (counter) {
        uint64_t c = 0;
        for (int i = 0; i < 8; i++) c = c << 8 | b[8 + i];
        *counter = c;
    }
    return NEB_OK;
}

}  // extern "C"
