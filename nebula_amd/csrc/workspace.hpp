// workspace.hpp — device scratch memory that batches on any stream share, one batch at a time: the
// mixed-key scheduler's, the transmit batch's, the receive coalescer's, the relay forward's. It grows
// with the largest batch seen and is otherwise reused; one event, `done`, follows its last user.
// Every batch (the caller holds the owner's mutex): reserve(bytes, &grew), begin(s), its launches on
// s, end(s). Host-only logic over a device policy, like queue_core.hpp: the engine binds it to HIP
// (HipWsApi below), tests/sanitize/workspace_test.cpp to a fake that logs the calls. Api has Stream,
// Event, Error, kOk, event_create / _sync / _record / _destroy, stream_wait, stream_id (0 = the
// runtime gives none), mem_alloc and mem_free; hip_owned.hpp's buffers add host_alloc and host_free;
// table_mirror.hpp's images add memset, copy_h2d (asynchronous, from pinned memory), stream_sync,
// device_sync, kPinned (the host_alloc flags of its staging) and event_create_host: an event the
// host waits for, with timing disabled and nothing else.
#pragma once

#include <cstddef>
#include <cstdint>

#include "hip_owned.hpp"

namespace neb {

// The stream a workspace's `done` event was last recorded on. A batch on that same stream is
// ordered after it already and skips the cross-stream wait (a barrier packet that cost ≈ 5 µs between
// kernels). The handle alone does not name a stream: one destroyed with work still pending is
// released when the work ends, and a stream created meanwhile may get its address; so the identity
// is the handle together with HIP's per-stream id (hipStreamGetId, HIP >= 7.1, looked up at run time:
// a process may run an older HIP runtime, as PyTorch's wheel does). Without it the handle alone is
// the identity, and a caller must not destroy a stream while the engine's batches on it are pending
// (streams).
template <class Api>
struct StreamTag {
    typename Api::Stream h{};
    unsigned long long id = 0;
    bool valid = false;
    bool same(typename Api::Stream s) const { return valid && h == s && Api::stream_id(s) == id; }
    void set(typename Api::Stream s) {
        h = s;
        id = Api::stream_id(s);
        valid = true;
    }
};

// N buffers ordered by one event (N = 2: the transmit batch's workspace and its host form's staging).
template <class Api, int N = 1>
struct DevWorkspace {
    using Error = typename Api::Error;
    DevWorkspace() = default;
    DevWorkspace(const DevWorkspace&) = delete;
    DevWorkspace& operator=(const DevWorkspace&) = delete;
    ~DevWorkspace() { destroy(); }

    uint8_t* mem(int b = 0) const { return buf_[b]; }
    size_t bytes(int b = 0) const { return buf_[b].bytes(); }
    // `done`, for a batch that binds it to its last kernel's dispatch instead of end()'s marker
    // (then end_bound()); null before the first begin()
    typename Api::Event event() const { return done_; }
    Error sync() { return done_ ? Api::event_sync(done_) : Api::kOk; }  // the host waits for the last batch

    // Capacity suffices: no device call at all. Otherwise the host waits for `done`, the buffer is
    // freed and allocated anew, and the caller lays its pointers out again (*grew). A failed
    // allocation leaves it empty, capacity 0.
    Error reserve(size_t bytes, bool* grew = nullptr, int b = 0) {
        if (grew) *grew = false;
        if (buf_[b] && bytes <= buf_[b].bytes()) return Api::kOk;
        const Error err = sync();  // the old buffer may still be in use
        if (err != Api::kOk) return err;
        buf_[b].reset();
        return buf_[b].reserve(bytes, grew);
    }
    // s waits for the last batch, unless that ran on s itself. `done` is created on first use,
    // ordering only (the host and other streams wait for the kernels, nobody reads the workspace
    // from the host): no system-scope cache release at each record.
    Error begin(typename Api::Stream s) {
        if (!done_) return Api::event_create(&done_);  // nothing recorded yet: no wait
        return last_.same(s) ? Api::kOk : Api::stream_wait(s, done_);
    }
    Error end(typename Api::Stream s) {
        const Error err = Api::event_record(done_, s);
        if (err == Api::kOk) last_.set(s);
        return err;
    }
    void end_bound(typename Api::Stream s) { last_.set(s); }  // the batch bound event() to its last kernel on s
    void destroy() {  // waits for the last batch; with the owner's device current
        if (done_) {
            (void)Api::event_sync(done_);
            Api::event_destroy(done_);
        }
        for (auto& b : buf_) b.reset();
        done_ = {};
        last_ = {};
    }

  private:
    OwnedBuf<Api> buf_[N];
    typename Api::Event done_{};
    StreamTag<Api> last_;  // the stream `done` was last recorded on
};

}  // namespace neb

#if defined(__HIPCC__)
#include <dlfcn.h>
#include <hip/hip_runtime.h>

namespace neb {

struct HipWsApi {
    using Stream = hipStream_t;
    using Event = hipEvent_t;
    using Error = hipError_t;
    static constexpr Error kOk = hipSuccess;
    static hipError_t event_create(hipEvent_t* ev) {
        return hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventDisableSystemFence);
    }
    static hipError_t event_sync(hipEvent_t ev) { return hipEventSynchronize(ev); }
    static hipError_t event_record(hipEvent_t ev, hipStream_t s) { return hipEventRecord(ev, s); }
    static void event_destroy(hipEvent_t ev) { (void)hipEventDestroy(ev); }
    static hipError_t stream_wait(hipStream_t s, hipEvent_t ev) { return hipStreamWaitEvent(s, ev, 0); }
    static unsigned long long stream_id(hipStream_t s) {
        using GetId = hipError_t (*)(hipStream_t, unsigned long long*);
        static const GetId get = (GetId)dlsym(RTLD_DEFAULT, "hipStreamGetId");
        unsigned long long v = 0;
        return get && get(s, &v) == hipSuccess ? v : 0ull;
    }
    static hipError_t mem_alloc(uint8_t** p, size_t bytes) { return hipMalloc((void**)p, bytes); }
    static void mem_free(uint8_t* p) { (void)hipFree(p); }
    static hipError_t host_alloc(uint8_t** p, size_t bytes, unsigned flags) { return hipHostMalloc((void**)p, bytes, flags); }
    static void host_free(uint8_t* p) { (void)hipHostFree(p); }
    static constexpr unsigned kPinned = hipHostMallocDefault;
    static hipError_t event_create_host(hipEvent_t* ev) { return hipEventCreateWithFlags(ev, hipEventDisableTiming); }
    static hipError_t memset(void* p, int v, size_t bytes) { return hipMemset(p, v, bytes); }
    static hipError_t copy_h2d(void* dst, const void* src, size_t bytes, hipStream_t s) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    }
    static hipError_t stream_sync(hipStream_t s) { return hipStreamSynchronize(s); }
    static hipError_t device_sync() { return hipDeviceSynchronize(); }
};
template <int N = 1>
using HipWorkspace = DevWorkspace<HipWsApi, N>;

}  // namespace neb
#endif
