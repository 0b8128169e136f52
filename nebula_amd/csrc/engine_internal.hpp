// engine_internal.hpp — what engine.cpp offers window.cpp and queue.cpp beside the C ABI
// (include/nebula_aead.h): one batch launch (neb::BatchLaunch, neb_launch), the host receive's
// staging (neb::RxStaging), the scheduler workspaces and a few accessors. Hidden symbols, declared
// here once, described at their definitions.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/nebula_aead.h"
#include "sched.hpp"
#include "workspace.hpp"  // (and hip_owned.hpp)

struct SchedSpace;  // the mixed-key scheduler's device workspace

namespace neb {

// One seal or open of a batch on a stream: everything the launch takes, by name (designated
// initializers, in this order). Pointers are device-addressable.
struct BatchLaunch {
    int alg = 0, open = 0;
    const neb_desc* desc = nullptr;
    uint32_t n = 0;
    const uint32_t* d_n = nullptr;  // optional: the real packet count in device memory, at most n
    uint8_t* arena = nullptr;
    int32_t* status = nullptr;
    uint32_t key_hint = NEB_KEYS_MIXED;
    hipStream_t stream = nullptr;
    SchedSpace* sched = nullptr;  // mixed-key AES-GCM: the workspace to bin in (null: the engine's)
    bool prebinned = false;       // ... which holds this batch's binning already (neb_rx_sched_begin)
    int hdr_from_dst = 0;         // tx.hip's descriptors: the first `flags` plaintext bytes come from dst
    hipEvent_t stop = nullptr;    // bound to the last kernel (single-key and ChaCha20 batches)
    const uint8_t* rx = nullptr;  // opens: the device receive's admission mask (rxwin.hip)
    bool note_use = false;        // neb_launch: a key-use marker behind the batch (neb_cipher_destroy)
};

// The host receive's zero-copy open (window.cpp): pinned descriptor and status staging and the
// engine's receive stream, reserved for the caller (e->rx.mu) while the object lives.
class RxStaging {
  public:
    // The caller has validated every descriptor. Not active with rc() == NEB_OK: not applicable (the
    // arena is not mapped pinned memory, the host mode is DMA, or n == 0); neb_open_batch_host then.
    RxStaging(neb_engine* e, int alg, uint32_t key_hint, uint8_t* arena, uint32_t n);
    ~RxStaging();  // waits for the receive stream, then releases the staging
    RxStaging(const RxStaging&) = delete;
    RxStaging& operator=(const RxStaging&) = delete;
    bool active() const { return e_ != nullptr; }
    int rc() const { return rc_; }
    neb_desc* desc() const { return desc_; }            // room for n descriptors
    const int32_t* status() const { return status_; }  // the statuses of open()'s descriptors
    int open(uint32_t cnt);  // the first cnt descriptors opened in the arena; returns when they are

  private:
    neb_engine* e_ = nullptr;
    int alg_, rc_;
    uint32_t key_hint_;
    uint8_t* arena_;
    neb_desc* desc_ = nullptr;
    int32_t* status_ = nullptr;
};

}  // namespace neb

extern "C" {
int neb_engine_device_of(const neb_engine* e);
int neb_check_batch_args(neb_engine* e, int alg, uint32_t key_hint);
int neb_key_alg(neb_engine* e, uint32_t key);
bool neb_host_mapped(const void* p);
void neb_engine_key_table(const neb_engine* e, const uint32_t** d_keys, uint32_t* max_keys);
SchedSpace* neb_sched_space_new();
void neb_sched_space_free(SchedSpace* sp);  // with the engine's device current
int neb_launch(neb_engine* e, const neb::BatchLaunch& b);
int neb_rx_sched_begin(neb_engine* e, uint32_t n, SchedSpace* sched, hipStream_t s, neb::SchedWs* ws,
                       uint32_t* max_keys);
void neb_rx_sched_abort(SchedSpace* sched);
}

struct SchedSpaceFree {
    void operator()(SchedSpace* sp) const { neb_sched_space_free(sp); }
};
using SchedSpacePtr = std::unique_ptr<SchedSpace, SchedSpaceFree>;  // (neb_sched_space_new())
