// hip_owned.hpp — owners of the host engine's HIP resources: a grow-only buffer (device or pinned
// host memory), an event and a stream. Each is move-only and releases in its destructor, so a struct
// of them needs no release list and an early return leaks nothing. They release with whatever
// device is current: the owner's destroy function sets its device (DeviceGuard), waits for its
// streams, and only then deletes the object. The buffer is host-only logic over workspace.hpp's
// device policy and runs on a fake device in tests/sanitize/owned_test.cpp; the handles are plain HIP.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

namespace neb {

// HostFlags < 0: device memory; otherwise pinned host memory allocated with those flags.
template <class Api, class T = uint8_t, int HostFlags = -1>
class OwnedBuf {
  public:
    using Error = typename Api::Error;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    ~OwnedBuf() { reset(); }  // (move construction only: nothing assigns one)

    operator T*() const { return reinterpret_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }  // the capacity

    // Capacity suffices: no device call at all. Otherwise the old block, if there is one, is freed
    // once wait() has returned kOk (whatever may still use it: the caller's stream, a set of
    // streams; its failure leaves the buffer as it was) and a block of `bytes` is allocated. A
    // failed allocation leaves the buffer empty, capacity 0, and a later reserve tries again.
    template <class Wait>
    Error reserve(size_t bytes, bool* grew, Wait&& wait) {
        if (grew) *grew = false;
        if (p_ && bytes <= bytes_) return Api::kOk;
        if (p_) {
            const Error err = wait();
            if (err != Api::kOk) return err;
            reset();
        }
        Error err;
        if constexpr (HostFlags < 0) err = Api::mem_alloc(&p_, bytes);
        else err = Api::host_alloc(&p_, bytes, (unsigned)HostFlags);
        if (err != Api::kOk) p_ = nullptr;
        else bytes_ = bytes;
        if (grew) *grew = err == Api::kOk;
        return err;
    }
    Error reserve(size_t bytes, bool* grew = nullptr) {  // nothing can be using the old block
        return reserve(bytes, grew, [] { return Api::kOk; });
    }
    void reset() {
        if (!p_) return;
        if constexpr (HostFlags < 0) Api::mem_free(p_);
        else Api::host_free(p_);
        p_ = nullptr;
        bytes_ = 0;
    }

  private:
    uint8_t* p_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace neb

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace neb {

struct HipWsApi;  // workspace.hpp
// PinnedBuf: hipHostMallocDefault (the device addresses it too); MappedBuf: hipHostMallocMapped
template <class T = uint8_t>
using DevBuf = OwnedBuf<HipWsApi, T>;
template <class T = uint8_t>
using PinnedBuf = OwnedBuf<HipWsApi, T, (int)hipHostMallocDefault>;
template <class T = uint8_t>
using MappedBuf = OwnedBuf<HipWsApi, T, (int)hipHostMallocMapped>;

template <class H, class Derived>
class HipHandle {
  public:
    HipHandle() = default;
    HipHandle(HipHandle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~HipHandle() {
        if (h_) Derived::destroy(h_);
    }
    operator H() const { return h_; }

  protected:
    H h_ = nullptr;
};

// The create calls fix the flags and do nothing for a handle that exists, so a set-up that failed
// half way is completed by calling it again.
struct Event : HipHandle<hipEvent_t, Event> {
    hipError_t create(unsigned flags) { return h_ ? hipSuccess : hipEventCreateWithFlags(&h_, flags); }
    static void destroy(hipEvent_t ev) { (void)hipEventDestroy(ev); }
};

struct Stream : HipHandle<hipStream_t, Stream> {
    hipError_t create(unsigned flags) { return h_ ? hipSuccess : hipStreamCreateWithFlags(&h_, flags); }
    hipError_t create_priority(unsigned flags, int priority) {
        return h_ ? hipSuccess : hipStreamCreateWithPriority(&h_, flags, priority);
    }
    hipError_t create_cu_mask(uint32_t words, const uint32_t* mask) {
        return h_ ? hipSuccess : hipExtStreamCreateWithCUMask(&h_, words, mask);
    }
    static void destroy(hipStream_t s) {  // what it still has queued runs first
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
};

}  // namespace neb
#endif
